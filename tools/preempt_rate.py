#!/usr/bin/env python3
"""Cost of the preemption dry run (kg_eval_preempt) by number of preemptors, on config 2's nodes (10k) and config 4's
(100k), about 30 generated resident pods per node (tests/preempt_ref.residents). Beside each case:
  port      the CPU reference loop (tests/preempt_ref.preempt over the oracle's verify rows; kind "port" as the other
            baselines: a restatement of the reference on the CPU, not the Go scheduler itself), one call
It imports the package of the tree it lies in and needs an MI355X; one process, one context.

Each case is timed with and without the victim masks downloaded, as the mean of `steps` synchronous calls after
--warmup, --repeat times (host clock from entry to the summaries on the host; every call ends in a stream
synchronise), the two legs alternating inside each repeat. The device's summaries and victim masks are compared with
the port's once per case, and the tool fails when they differ.
Per cluster it also reports the time of the table's upload (kg_snapshot_upload_residents, one call) and of replacing
one node's list (kg_snapshot_update_residents, 20 calls after the warm-up).

    python tools/preempt_rate.py [--warmup 2] [--repeat 3] [--commit ID] [--out FILE]

Prints one JSON object and writes it to --out (default profiles/preempt/preempt_rate.json)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PREEMPTORS = (1, 16, 100)
PRIORITY = 6000  # above four of the residents' five levels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--configs", default="2,4")
    ap.add_argument("--preemptors", default=",".join(map(str, PREEMPTORS)))
    ap.add_argument("--per-node", type=int, default=30)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "preempt", "preempt_rate.json"))
    a = ap.parse_args()

    import numpy as np

    import preempt_ref
    from koordinator_amd import abi, engine, synth

    ctx = engine.Context(0)

    def stats(v, steps):
        return {"ms": v, "median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "steps": steps}

    def timed(legs, steps):
        for fn in legs.values():
            for _ in range(a.warmup):
                fn()
        ctx.sync()
        ms = {k: [] for k in legs}
        for _ in range(a.repeat):
            for k, fn in legs.items():
                t0 = time.perf_counter()
                for _ in range(steps):
                    fn()
                ctx.sync()
                ms[k].append((time.perf_counter() - t0) / steps * 1e3)
        return {k: stats(v, steps) for k, v in ms.items()}

    result = {"commit": a.commit, "warmup": a.warmup, "repeat": a.repeat, "per_node": a.per_node, "priority": PRIORITY,
              "timing": "host clock around synchronous calls, mean per call over `steps` calls; the two device legs "
                        "alternate per repeat; the port: one call",
              "clusters": {}}
    fields = [f for f in abi.PREEMPT_NODE_DTYPE.names if f != "pad_"]
    for config in [int(x) for x in a.configs.split(",")]:
        cfg, nodes, pods = synth.cluster(config)
        kc = cfg.kg_config()
        batch = engine.PodBatch(ctx, pods)
        snap = engine.Snapshot(ctx, kc, nodes)
        res = preempt_ref.residents(nodes, 5, per_node=a.per_node)
        t0 = time.perf_counter()
        snap.upload_residents(res)
        upload_ms = (time.perf_counter() - t0) * 1e3
        # what a caller does after a bind: one node's list replaced (by itself here, so the table stays what it was)
        one = {k: v[res["node"] == 0].copy() for k, v in res.items()}
        update_ms = []
        for _ in range(a.warmup + 20):
            t0 = time.perf_counter()
            snap.update_residents([0], one)
            update_ms.append((time.perf_counter() - t0) * 1e3)
        update_ms = update_ms[a.warmup:]
        cases = {}
        for n in [int(x) for x in a.preemptors.split(",")]:
            rows = (np.arange(n, dtype=np.uint64) * batch.n // n).astype(np.uint32)
            prio = np.full(n, PRIORITY, np.int32)
            t0 = time.perf_counter()
            want = preempt_ref.preempt(kc, nodes, pods, res, rows, prio, None)
            port_ms = (time.perf_counter() - t0) * 1e3
            got = engine.eval_preempt(snap, batch, rows, prio, None, preempt_ref.ALLOWED, 0, victims=True)
            equal = all(np.array_equal(got[0][f], want[0][f]) for f in fields) and np.array_equal(got[1], want[1])
            r = {"n_rows": n, "equal_port": bool(equal), "pairs": n * snap.n,
                 "results": np.bincount(want[0]["result"].ravel(), minlength=5).tolist(),
                 "mean_potential": float(want[0]["n_potential"].mean()), "max_victims": int(want[0]["n_victims"].max()),
                 "port": dict(stats([port_ms], 1), kind="port")}
            steps = max(3, min(50, 4_000_000 // (n * snap.n)))
            r.update(timed({
                "summaries": lambda: engine.eval_preempt(snap, batch, rows, prio, None, preempt_ref.ALLOWED, 0),
                "with_masks": lambda: engine.eval_preempt(snap, batch, rows, prio, None, preempt_ref.ALLOWED, 0, victims=True),
            }, steps))
            cases[str(n)] = r
            print(f"config{config} preemptors={n}: " + ", ".join(
                f"{k}={v['median_ms']:.3f}" for k, v in r.items() if isinstance(v, dict)) + f" equal_port={equal}",
                  file=sys.stderr, flush=True)
            if not equal:
                raise SystemExit(f"config{config}, {n} preemptors: the device differs from the port")
        result["clusters"][f"config{config}"] = {"n_nodes": snap.n, "n_pods": batch.n, "residents": abi.table_len(res),
                                                 "upload_residents_ms": upload_ms, "update_one_node": stats(update_ms, 1),
                                                 "preemptors": cases}
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
