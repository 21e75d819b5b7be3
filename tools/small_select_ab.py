#!/usr/bin/env python3
"""A/B aid for the one-pod-block fused top-1 select (k_select_small, finishing in its own launch or followed by
k_small_finish; select_small in kg_runtime.cpp) under bench.py's warm-up and step counts. It imports the package of the tree it lies in.

Default: config 2's pods (145 distinct rows of 10,000) against config 2's nodes and against synth.mixed()'s nodes,
which hold many F_BIG records (Restricted nodes, node CPU bind policies: the records the new path evaluates inline
instead of in k_big_sel), each timed on the one-launch path, with KG_NO_SMALL_FUSED_FINISH=1 (the two launches) and
with KG_NO_SMALL_SELECT=1 (the general path) in the same process, alternating; the keys of the paths are compared once
per snapshot.

--sweep "c0,c1,copies;...": the new path under KG_SMALL_CHUNKS settings (records per workgroup of storage class 0 / 1,
lane copies per workgroup: up to 512 threads run the launch-bound variant without scratch), what select_small's
geometry is set from.
--nodes also takes config4 (100,000 nodes).
--lanes N: N all-distinct pods instead of config 2's (the launch then has N lanes, no pod-row reduction).
--rows N: config 2's pods tiled to N rows (the same distinct rows: the lane count stays, the finish writes N rows), for
the row gate of the one-launch finish in select_small.
--replicas "1,4,...,all,two": the one-launch path under KG_SMALL_REPLICAS settings ("all": one replica per chunk, no two
workgroups share an address; "two": KG_NO_SMALL_FUSED_FINISH=1, the two launches, as the yardstick), what select_small's
replica rule is set from.
--profile: the timed loop runs with the profile bracket on, as bench.py's does; every line also carries the host time of
the submission loop alone (submit_ms_small: per call, before the final sync) and the bracket's device time per select.
--bracket clock|events (with --profile): the one-launch select times itself with the device clock (the default) or
keeps the event pair bound to its launch (KG_PROFILE_BOUND_EVENTS=1); every line says which bracket it used.
--phases: where the one-launch kernel's time goes (KG_SMALL_PHASES: the kernel's instantiation that stores four clock
readings per workgroup; config 2's shape only). One JSON line per snapshot: medians over workgroups and steps of the
time from the launch's earliest entry to each workgroup's entry, loops done and ticket drawn, and to the finisher's end.
In the default form (the accumulators are the result, no finisher) the third reading is "result atomics complete" and
the fourth the same reading's successor in the workgroup that was last: the launch's end; the fields keep their names
(ticket_* = atomics complete, finisher_end = end of launch). tail_us = end of launch - slowest workgroup's loops.
--finisher: KG_SMALL_FINISHER=1 for the whole run, the lane form with its finisher (the form before; A/B yardstick).
--shares "0,0.02,...": synth.mixed()'s nodes thinned to these F_BIG shares (every other node kept, the first F_BIG
nodes up to the share), for the break-even of the F_BIG gate in select_small. KG_SMALL_ALLOW_BIG=1 (set here) lifts
that gate so that both paths can be timed above it.

    python tools/small_select_ab.py [--steps 20] [--warmup 3] [--repeat 3] [--nodes config2,mixed] [--sweep ...]

Prints one JSON line per (nodes, setting, repeat)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--nodes", default="config2,mixed")
    ap.add_argument("--sweep", default=None)
    ap.add_argument("--lanes", type=int, default=0)
    ap.add_argument("--rows", type=int, default=0)
    ap.add_argument("--replicas", default=None)
    ap.add_argument("--shares", default=None)
    ap.add_argument("--chunks", default=None, help="KG_SMALL_CHUNKS for the new path's side of the A/B")
    ap.add_argument("--profile", action="store_true",
                    help="time with the profile bracket on (ctx.profile, as bench.py does) and report the bracket")
    ap.add_argument("--bracket", choices=["clock", "events"], default="clock",
                    help="with --profile: the one-launch select's bracket (device clock inside the launch / bound event pair)")
    ap.add_argument("--phases", action="store_true", help="per-workgroup phase times of the one-launch kernel")
    ap.add_argument("--finisher", action="store_true", help="KG_SMALL_FINISHER=1: the lane form with its finisher")
    a = ap.parse_args()
    if a.finisher:
        os.environ["KG_SMALL_FINISHER"] = "1"
    else:
        os.environ.pop("KG_SMALL_FINISHER", None)
    if a.bracket == "events":
        os.environ["KG_PROFILE_BOUND_EVENTS"] = "1"
    else:
        os.environ.pop("KG_PROFILE_BOUND_EVENTS", None)

    import numpy as np

    from koordinator_amd import abi, engine, synth

    cfg, nodes2, pods = synth.cluster(2)
    if a.lanes:
        pods = abi.take(pods, np.arange(a.lanes))
        pods["req_eph"] = (pods["req_eph"] + np.arange(a.lanes)).astype(np.int64)
    if a.rows:
        pods = abi.take(pods, np.arange(a.rows) % abi.table_len(pods))
    ctx = engine.Context(0)
    batch = engine.PodBatch(ctx, pods)
    lanes = batch.select_lanes()

    last = {}  # of the latest time_select: host time of the submission loop alone, and the profile bracket

    def time_select(snap):
        for _ in range(a.warmup):
            engine.eval_select_async(snap, batch, 1)
        ctx.sync()
        if a.profile:  # as bench.py does around its timed steps
            ctx.profile(True)
            ctx.profile_read(reset=True)
            ctx.sync()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            engine.eval_select_async(snap, batch, 1)
        t1 = time.perf_counter()
        ctx.sync()
        t2 = time.perf_counter()
        last["submit_ms"] = (t1 - t0) / a.steps * 1e3
        last["bracket_ms"] = None
        if a.profile:
            ms, n = ctx.profile_read(reset=True)
            ctx.profile(False)
            last["bracket_ms"] = ms / n if n else None
        return (t2 - t0) / a.steps * 1e3

    def phases_of(snap):
        """Median microseconds (100 MHz device clock) over a.steps launches, each read from the KG_SMALL_PHASES file."""
        import tempfile
        fd, path = tempfile.mkstemp(suffix=".phases")
        os.close(fd)
        for _ in range(a.warmup):
            engine.eval_select_async(snap, batch, 1)
        ctx.sync()
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
        per, at = [], 0
        while at < len(raw):
            nc = int(raw[at])
            t = raw[at + 1:at + 1 + 4 * nc].reshape(nc, 4).astype(np.int64)
            at += 1 + 4 * nc
            t0 = t[:, 0].min()
            fin = t[t[:, 3] != 0]
            assert len(fin) == 1, "one finisher (or last workgroup) per launch"
            per.append(dict(workgroups=nc, entry=np.median(t[:, 0] - t0), entry_max=(t[:, 0] - t0).max(),
                            loops=np.median(t[:, 1] - t0), loops_max=(t[:, 1] - t0).max(),
                            ticket=np.median(t[:, 2] - t0), ticket_max=(t[:, 2] - t0).max(),
                            loops_own=np.median(t[:, 1] - t[:, 0]), ticket_own=np.median(t[:, 2] - t[:, 1]),
                            finisher_ticket=fin[0, 2] - t0, finisher_end=fin[0, 3] - t0, finisher_own=fin[0, 3] - fin[0, 2],
                            tail=fin[0, 3] - t[:, 1].max()))
        if not per:
            return None
        return {k + ("_us" if k != "workgroups" else ""): float(np.median([q[k] for q in per])) / (1.0 if k == "workgroups" else 100.0)
                for k in per[0]} | {"launches": len(per)}

    def with_env(name, value, fn):
        os.environ[name] = value
        try:
            return fn()
        finally:
            del os.environ[name]

    def big_of(nodes):
        big = nodes["numa_policy"] == abi.KG_NUMA_RESTRICTED
        if "cpu_bind_policy" in nodes:
            big = big | (nodes["cpu_bind_policy"] != 0)
        return big

    os.environ["KG_SMALL_ALLOW_BIG"] = "1"
    sets = [(name, nodes2 if name == "config2" else synth.cluster(4)[1] if name == "config4" else synth.mixed()[1])
            for name in a.nodes.split(",")]
    if a.shares:
        mixed = synth.mixed()[1]
        mbig = big_of(mixed)
        rest, bigs = np.flatnonzero(~mbig), np.flatnonzero(mbig)
        sets = []
        for sh in (float(x) for x in a.shares.split(",")):
            k = min(len(bigs), int(round(sh * len(rest) / (1.0 - sh))))
            sets.append((f"mixed_share_{sh}", abi.take(mixed, np.sort(np.concatenate([rest, bigs[:k]])))))
    for name, nodes in sets:
        big = big_of(nodes)
        snap = engine.Snapshot(ctx, cfg.kg_config(), nodes)
        keys = engine.eval_select(snap, batch, 1)
        keys0 = with_env("KG_NO_SMALL_SELECT", "1", lambda: engine.eval_select(snap, batch, 1))
        keys2 = with_env("KG_NO_SMALL_FUSED_FINISH", "1", lambda: engine.eval_select(snap, batch, 1))
        head = {"form": "finisher" if a.finisher else "default", "nodes": name, "n_nodes": abi.table_len(nodes), "f_big_share": float(big.mean()), "pods": batch.n,
                "lanes": lanes[0], "fast_lanes": lanes[1], "steps": a.steps, "warmup": a.warmup,
                "keys_equal": bool(np.array_equal(keys, keys0)), "keys_equal_two_launch": bool(np.array_equal(keys, keys2)),
                "feasible_rows": int((keys != 0).sum())}

        def time_replicas(r):
            if r == "two":
                return with_env("KG_NO_SMALL_FUSED_FINISH", "1", lambda: time_select(snap))
            return with_env("KG_SMALL_REPLICAS", "4096" if r == "all" else r, lambda: time_select(snap))

        if a.phases:
            print(json.dumps(dict(head, phases=phases_of(snap), unit="us from the launch's earliest workgroup entry, medians "
                                  "over workgroups, then over launches (*_own: within the workgroup)")), flush=True)
            snap.close()
            continue
        for rep in range(a.repeat):
            if a.replicas:
                for r in a.replicas.split(","):
                    ms = with_env("KG_SMALL_CHUNKS", a.chunks, lambda: time_replicas(r)) if a.chunks else time_replicas(r)
                    print(json.dumps(dict(head, repeat=rep, chunks=a.chunks, replicas=r, select_ms_small=ms,
                                          profile=a.profile, bracket=a.bracket if a.profile and r != "two" else
                                          "events" if a.profile else None, submit_ms_small=last["submit_ms"],
                                          bracket_ms_small=last["bracket_ms"])), flush=True)
            elif a.sweep:
                for setting in a.sweep.split(";"):
                    ms = with_env("KG_SMALL_CHUNKS", setting, lambda: time_select(snap))
                    print(json.dumps(dict(head, repeat=rep, chunks=setting, select_ms_small=ms)), flush=True)
            else:
                small = with_env("KG_SMALL_CHUNKS", a.chunks, lambda: time_select(snap)) if a.chunks else time_select(snap)
                host = dict(profile=a.profile, bracket=a.bracket if a.profile else None, submit_ms_small=last["submit_ms"], bracket_ms_small=last["bracket_ms"])
                two = with_env("KG_NO_SMALL_FUSED_FINISH", "1", lambda: time_select(snap))
                general = with_env("KG_NO_SMALL_SELECT", "1", lambda: time_select(snap))
                print(json.dumps(dict(head, repeat=rep, chunks=a.chunks, select_ms_small=small, select_ms_two_launch=two,
                                      select_ms_general=general, **host)), flush=True)
        snap.close()
    batch.close()
    ctx.close()


if __name__ == "__main__":
    main()
