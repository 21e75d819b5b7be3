#!/usr/bin/env python3
"""Per-workgroup phase times of the one-launch top-1 select (k_select_small) on config 2, by storage class and chunk:
what tools/small_select_ab.py --phases folds into medians over all workgroups. KG_SMALL_PHASES (kg_runtime.cpp) makes
every launch append four device-clock readings per workgroup; here they are taken per chunk as medians over the
launches. KG_SMALL_CHUNKS="c0,c1,copies" in the caller's environment sets the geometry, as for the library.

    python tools/small_phases_by_chunk.py [--steps 20] [--all]

Prints the loop time (entry to loops done) per storage class, the entry times, the workgroups that are through last,
and with --all both series for every chunk (class-1 chunks first, as the kernel numbers them). The third reading is
"result atomics complete" in the default form, which has no finisher, and "ticket drawn" under KG_SMALL_FINISHER=1; the
fourth is set in one workgroup, the last one through: the launch's end."""
import argparse
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--all", action="store_true")
    a = ap.parse_args()

    import numpy as np

    from koordinator_amd import abi, engine, synth

    cfg, nodes, pods = synth.cluster(2)
    ctx = engine.Context(0)
    snap = engine.Snapshot(ctx, cfg.kg_config(), nodes)
    batch = engine.PodBatch(ctx, pods)
    n1 = int((nodes["numa_policy"] == abi.KG_NUMA_SINGLE_NODE).sum())
    for _ in range(3):
        engine.eval_select_async(snap, batch, 1)
    ctx.sync()
    fd, path = tempfile.mkstemp(suffix=".phases")
    os.close(fd)
    os.environ["KG_SMALL_PHASES"] = path
    try:
        for _ in range(a.steps):
            engine.eval_select_async(snap, batch, 1)
        ctx.sync()
    finally:
        del os.environ["KG_SMALL_PHASES"]
    raw = np.fromfile(path, dtype=np.uint64)
    os.remove(path)
    if os.path.exists(path + ".ops"):  # the fifth reading's file (tools/small_prologue.py reads it)
        os.remove(path + ".ops")
    nc = int(raw[0])
    t = raw.reshape(a.steps, 1 + 4 * nc)[:, 1:].reshape(a.steps, nc, 4).astype(np.int64)
    t0 = t[:, :, 0].min(axis=1)[:, None]
    entry = np.median(t[:, :, 0] - t0, axis=0) / 100
    own = np.median(t[:, :, 1] - t[:, :, 0], axis=0) / 100
    done = np.median(t[:, :, 1] - t0, axis=0) / 100
    third = np.median(t[:, :, 2] - t0, axis=0) / 100
    end = np.median(t[:, :, 3].max(axis=1) - t0[:, 0]) / 100
    name3 = "ticket drawn" if os.environ.get("KG_SMALL_FINISHER") else "result atomics complete"
    # the kernel numbers the class-1 chunks first; how many there are follows from the class-1 chunk length
    setting = os.environ.get("KG_SMALL_CHUNKS")
    if not setting:
        raise SystemExit("set KG_SMALL_CHUNKS=c0,c1,copies (the geometry to look at)")
    c1 = int(setting.split(",")[1])
    nc1 = -(-n1 // c1)
    print(f"workgroups {nc}, class-1 chunks {nc1} of {c1} records (us, medians over {a.steps} launches)")
    print("loops, class 1: median %.2f max %.2f; class 0: median %.2f max %.2f" %
          (np.median(own[:nc1]), own[:nc1].max(), np.median(own[nc1:]), own[nc1:].max()))
    print("entry, class 1: median %.2f max %.2f; class 0: median %.2f max %.2f" %
          (np.median(entry[:nc1]), entry[:nc1].max(), np.median(entry[nc1:]), entry[nc1:].max()))
    print("%s: median %.2f max %.2f; end of launch %.2f, %.2f behind the slowest workgroup's loops" %
          (name3, np.median(third), third.max(), end, end - done.max()))
    print("through last (chunk, entry, loops, loops done, %s):" % name3)
    for c in np.argsort(-done)[:8]:
        print("  %d %.2f %.2f %.2f %.2f" % (c, entry[c], own[c], done[c], third[c]))
    if a.all:
        print("loops by chunk:", " ".join("%.1f" % x for x in own))
        print("entry by chunk:", " ".join("%.1f" % x for x in entry))
    batch.close()
    snap.close()
    ctx.close()


if __name__ == "__main__":
    main()
