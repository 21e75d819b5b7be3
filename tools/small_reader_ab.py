#!/usr/bin/env python3
"""What a caller of the one-launch top-1 select pays end to end: kg_eval_select followed by kg_result_keys and
kg_result_status, per call, with the stream idle before each call. The lane form of the result (select_local in
kg_runtime.cpp) moves the expansion of the rows from the launch's lone finisher to the two readers, which gather on the
host; this tool shows whether the readers pay back what the launch saves.

Config 2's nodes and pods, the pods tiled to --rows rows (the same 145 distinct rows, as small_select_ab.py --rows).
Per row count and repeat one JSON line: median and minimum over --steps calls of the whole cycle (cycle_ms), of its
select part up to the stream's sync (select_sync_ms: a second loop, select + sync only) and of the two reads after a
synchronised select (read_ms), plus the pipelined select-only time per step as bench.py measures it (select_ms: --steps
selects back to back, one sync). --row-form sets KG_SMALL_ROW_RESULTS=1 (this tree's row form). --tree DIR imports the
package of another checkout, for a side-by-side run against the parent commit.

    python tools/small_reader_ab.py [--rows 10000,50000,200000] [--steps 200] [--warmup 20] [--repeat 5] [--tree DIR]"""
import argparse
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="10000,50000,200000")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--row-form", action="store_true")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--label", default="this", help="the record's \"tree\" field")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    if a.row_form:
        os.environ["KG_SMALL_ROW_RESULTS"] = "1"

    import numpy as np

    from koordinator_amd import abi, engine, synth

    cfg, nodes, pods0 = synth.cluster(2)
    ctx = engine.Context(0)
    snap = engine.Snapshot(ctx, cfg.kg_config(), nodes)

    def stats(ts):
        return {"median": float(np.median(ts)) * 1e3, "min": float(np.min(ts)) * 1e3}

    for rows in (int(x) for x in a.rows.split(",")):
        pods = abi.take(pods0, np.arange(rows) % abi.table_len(pods0))
        batch = engine.PodBatch(ctx, pods)
        want = engine.eval_select(snap, batch, 1)
        for rep in range(a.repeat):
            cycle, sel, rd = [], [], []
            for i in range(a.warmup + a.steps):
                ctx.sync()
                t0 = time.perf_counter()
                engine.eval_select_async(snap, batch, 1)
                keys = engine.result_keys(batch, 1)
                status = engine.result_status(batch)
                t1 = time.perf_counter()
                if i >= a.warmup:
                    cycle.append(t1 - t0)
            same = bool(np.array_equal(keys, want)) and not status.any()
            for i in range(a.warmup + a.steps):
                ctx.sync()
                t0 = time.perf_counter()
                engine.eval_select_async(snap, batch, 1)
                ctx.sync()
                t1 = time.perf_counter()
                engine.result_keys(batch, 1)
                engine.result_status(batch)
                t2 = time.perf_counter()
                if i >= a.warmup:
                    sel.append(t1 - t0)
                    rd.append(t2 - t1)
            for _ in range(a.warmup):
                engine.eval_select_async(snap, batch, 1)
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                engine.eval_select_async(snap, batch, 1)
            ctx.sync()
            piped = (time.perf_counter() - t0) / a.steps * 1e3
            print(json.dumps({"tree": a.label, "row_form": a.row_form, "rows": rows,
                              "lanes": batch.select_lanes()[0], "repeat": rep, "steps": a.steps, "results_equal": same,
                              "cycle_ms": stats(cycle), "select_sync_ms": stats(sel), "read_ms": stats(rd),
                              "select_ms": piped}), flush=True)
        batch.close()
    snap.close()
    ctx.close()


if __name__ == "__main__":
    main()
