#!/usr/bin/env python3
"""Cost of the node offer slots (kg_eval_offer_slots) by gang size, on config 2's nodes (10k) and config 4's (100k).
There is no other device route to the counts, so two neighbours are reported beside it:
  port      the CPU reference loop (tests/offer_slots_ref.offer_slots over the oracle's verify rows; kind "port" as the
            other baselines: a restatement of the reference on the CPU, not the Go scheduler itself), a few calls
  feasible  kg_eval_feasible of the same rows: the same pairs at most, one Filter each, no accumulation: the floor
It imports the package of the tree it lies in and needs an MI355X; one process, one context.

Two gangs per size: `copies` (n copies of one pod, the gang of identical pods: the longest loops, a node runs until
it is full) and `spread` (n distinct pods evenly spread over the batch: most nodes stop early). Timed per case as the
mean of `steps` synchronous calls after --warmup, --repeat times (host clock from entry to the counts on the host;
every call ends in a stream synchronise), the device legs alternating inside each repeat. The device's counts and
status words are compared with the port's once per case.

    python tools/offer_slots_rate.py [--warmup 3] [--repeat 3] [--commit ID] [--out FILE]

Prints one JSON object and writes it to --out (default profiles/offer_slots/offer_slots_rate.json)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

GANGS = (8, 64, 512)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--port-repeat", type=int, default=3)
    ap.add_argument("--configs", default="2,4")
    ap.add_argument("--gangs", default=",".join(map(str, GANGS)))
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "offer_slots", "offer_slots_rate.json"))
    a = ap.parse_args()

    import numpy as np

    import offer_slots_ref
    from koordinator_amd import engine, synth

    ctx = engine.Context(0)

    def stats(v, steps):
        return {"ms": v, "median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "steps": steps}

    def timed(legs):
        for fn in legs.values():
            for _ in range(a.warmup):
                fn()
        ctx.sync()
        ms = {k: [] for k in legs}
        for _ in range(a.repeat):
            for k, fn in legs.items():
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    fn()
                ctx.sync()
                ms[k].append((time.perf_counter() - t0) / a.steps * 1e3)
        return {k: stats(v, a.steps) for k, v in ms.items()}

    result = {"commit": a.commit, "warmup": a.warmup, "repeat": a.repeat,
              "timing": "host clock around synchronous calls, mean per call over `steps` calls; device legs alternate "
                        "per repeat; the port: one call per repeat",
              "clusters": {}}
    for config in [int(x) for x in a.configs.split(",")]:
        cfg, nodes, pods = synth.cluster(config)
        kc = cfg.kg_config()
        batch = engine.PodBatch(ctx, pods)
        snap = engine.Snapshot(ctx, kc, nodes)
        cases = {}
        for n in [int(x) for x in a.gangs.split(",")]:
            gangs = {"copies": np.full(n, 3, np.uint32),
                     "spread": (np.arange(n, dtype=np.uint64) * batch.n // n).astype(np.uint32)}
            for kind, rows in gangs.items():
                r = {"n_rows": n, "gang": kind}
                port_ms = []
                for _ in range(a.port_repeat):
                    t0 = time.perf_counter()
                    want = offer_slots_ref.offer_slots(kc, nodes, pods, rows)
                    port_ms.append((time.perf_counter() - t0) * 1e3)
                got = engine.eval_offer_slots(snap, batch, rows, status=True)
                r["equal_port"] = bool(np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]))
                r["pairs_evaluated"] = int(np.minimum(want[0].astype(np.int64) + 1, n).sum())
                r["pairs_flat"] = n * snap.n
                r["mean_slots"] = float(want[0].mean())
                r["max_slots"] = int(want[0].max())
                r["port"] = dict(stats(port_ms, 1), kind="port")
                r.update(timed({"offer_slots": lambda: engine.eval_offer_slots(snap, batch, rows, status=True),
                                "feasible": lambda: engine.eval_feasible(snap, batch, rows)}))
                cases[f"{n}_{kind}"] = r
                print(f"config{config} gang={n} {kind}: " + ", ".join(
                    f"{k}={v['median_ms']:.3f}" for k, v in r.items() if isinstance(v, dict)) +
                      f" equal_port={r['equal_port']}", file=sys.stderr, flush=True)
        result["clusters"][f"config{config}"] = {"n_nodes": snap.n, "n_pods": batch.n, "gangs": cases}
        snap.close()
        batch.close()
    ctx.close()
    text = json.dumps(result, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
