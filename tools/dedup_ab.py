#!/usr/bin/env python3
"""A/B aid for the plain select's pod-row deduplication, on bench config 2's nodes under bench.py's warm-up and step
counts. It imports the package of the tree it lies in, so copy it into the tree to be measured.

Default: times eval_select_async and PodBatch.upload for config 2's pods (145 distinct rows of 10,000) and for the same
pods made all-distinct (req_eph += j). Run it on two builds and compare: the all-distinct select takes the same device
path on both; its upload pays the row hashing.

--breakeven: batches whose duplicates save only a few 64-lane waves (all-distinct pods with the last m rows copies of
one row), each timed with the reduction on and with KG_NO_POD_DEDUP=1 in the same process: what the gate's threshold
in kg_runtime.cpp (dedup_on) is set from.

    python tools/dedup_ab.py [--steps 20] [--warmup 3] [--repeat 3] [--breakeven]

Prints one JSON line per (batch, repeat); "build" says whether the library has kg_pods_select_lanes."""
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
    ap.add_argument("--breakeven", action="store_true")
    a = ap.parse_args()

    import numpy as np

    from koordinator_amd import abi, engine, synth

    build = "dedup" if hasattr(engine.PodBatch, "select_lanes") else "no-dedup"
    cfg, nodes, pods = synth.cluster(2)
    n = abi.table_len(pods)
    distinct = {k: v.copy() for k, v in pods.items()}
    distinct["req_eph"] = (distinct["req_eph"] + np.arange(n)).astype(np.int64)
    ctx = engine.Context(0)
    snap = engine.Snapshot(ctx, cfg.kg_config(), nodes)

    def time_select(batch):
        for _ in range(a.warmup):
            engine.eval_select_async(snap, batch, 1)
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            engine.eval_select_async(snap, batch, 1)
        ctx.sync()
        return (time.perf_counter() - t0) / a.steps * 1e3

    def time_upload(batch, table):
        for _ in range(a.warmup):
            batch.upload(table)
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            batch.upload(table)
        ctx.sync()
        return (time.perf_counter() - t0) / a.steps * 1e3

    def waves(lanes, fast):
        return (fast + 63) // 64 + (lanes - fast + 63) // 64

    if not a.breakeven:
        for name, table in (("config2", pods), ("all_distinct", distinct)):
            batch = engine.PodBatch(ctx, table)
            lanes = batch.select_lanes()[0] if build == "dedup" else batch.n
            for rep in range(a.repeat):
                print(json.dumps({"build": build, "batch": name, "pods": batch.n, "lanes": lanes, "repeat": rep,
                                  "steps": a.steps, "warmup": a.warmup, "select_ms_per_step": time_select(batch),
                                  "upload_ms": time_upload(batch, table)}), flush=True)
            batch.close()
    else:
        cases = [(rows, m) for rows in (10000, 2560, 300) for m in (64, 128, 256, 512, 1024) if m < rows] + \
                [(300, 50), (300, 150)]
        for rows, m in cases:
            idx = np.arange(rows)
            idx[rows - m:] = rows - m - 1  # the last m rows repeat one row: m lanes fewer
            table = abi.take(distinct, idx)
            batch = engine.PodBatch(ctx, table)
            os.environ["KG_NO_POD_DEDUP"] = "1"
            full = waves(*batch.select_lanes())
            del os.environ["KG_NO_POD_DEDUP"]
            reduced = waves(*batch.select_lanes())  # what the select launches (the full list when the gate is off)
            for rep in range(a.repeat):
                on = time_select(batch)
                os.environ["KG_NO_POD_DEDUP"] = "1"
                off = time_select(batch)
                del os.environ["KG_NO_POD_DEDUP"]
                print(json.dumps({"build": build, "batch": f"{rows}_rows_{m}_copies", "waves_full": full,
                                  "waves_launched": reduced, "repeat": rep, "steps": a.steps, "warmup": a.warmup,
                                  "select_ms_dedup": on, "select_ms_no_dedup": off}), flush=True)
            batch.close()
    snap.close()
    ctx.close()


if __name__ == "__main__":
    main()
