#!/usr/bin/env python3
"""Cost of the feasible-node bitmaps (kg_eval_feasible) by row count and step-1 form, against the two neighbouring
calls on the same rows: kg_eval_verify with only the status matrix downloaded (the only other way to the per-pair
Filter results) and kg_eval_diagnose (the same pairs evaluated, counts instead of bits). It imports the package of the
tree it lies in and needs an MI355X; one process, one context.

Timed per case, each as the mean of `steps` synchronous calls after --warmup, --repeat times (host clock from entry to
the bitmap on the host; every call ends in a stream synchronise), the legs of one case alternating inside each repeat:
  feasible_rows / feasible_records   eval_feasible with KG_FEASIBLE_FORM forced
  feasible_default                   eval_feasible as shipped (the form follows FEAS_ROWS_MIN of kg_feasible.h)
  diagnose                           eval_diagnose of the same rows (first_plugin=False)
  verify_status                      eval_verify (status only) of a batch holding just those rows: kernel + download
                                     of the matrix; building that batch is not timed. Left out (with the reason in
                                     the output) above --verify-pairs pairs: the matrix alone is 4 bytes a pair on the
                                     host and 37 on the device
on config 2's cluster (10k pods x 10k nodes) and config 4's (10k pods x 100k nodes) with 1, 8, 64, 100, 1000 and all
10000 rows. Steps shrink with the pair count (--pairs-per-window, --verify-pairs-per-window) so that no leg takes
minutes. The bitmaps of both forms are compared with the verify route's status matrix once per case where that route
runs.

    python tools/feasible_rate.py [--warmup 2] [--repeat 3] [--commit ID] [--out FILE]

Prints one JSON object and writes it to --out (default profiles/feasible/feasible_rate.json)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROW_COUNTS = (1, 8, 64, 100, 1000, 10000)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--max-steps", type=int, default=400)
    ap.add_argument("--pairs-per-window", type=float, default=2e10, help="pairs one timed window evaluates at most")
    ap.add_argument("--verify-pairs-per-window", type=float, default=4e8, help="the same for the verify leg")
    ap.add_argument("--verify-pairs", type=float, default=1e8, help="largest verify matrix timed")
    ap.add_argument("--configs", default="2,4")
    ap.add_argument("--rows", default=",".join(map(str, ROW_COUNTS)))
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feasible", "feasible_rate.json"))
    a = ap.parse_args()

    import numpy as np

    from koordinator_amd import abi, engine, nodesets, synth

    ctx = engine.Context(0)

    def form(name):
        if name is None:
            os.environ.pop("KG_FEASIBLE_FORM", None)
        else:
            os.environ["KG_FEASIBLE_FORM"] = name  # read per call by the library

    def status_only(snap, batch):
        st = np.zeros((batch.n, snap.n), np.uint32)
        out = abi.KgVerifyOut()
        out.status = st.ctypes.data_as(C.POINTER(C.c_uint32))
        snap.ctx.check(snap.ctx.L.kg_eval_verify(snap.h, batch.h, C.byref(out)), "kg_eval_verify")
        return st

    def timed(legs):
        """legs: {name: (fn, steps)}. Per repeat every leg runs one window of its `steps` calls, in turn."""
        for fn, _ in legs.values():
            for _ in range(a.warmup):
                fn()
        ctx.sync()
        ms = {k: [] for k in legs}
        for _ in range(a.repeat):
            for k, (fn, steps) in legs.items():
                t0 = time.perf_counter()
                for _ in range(steps):
                    fn()
                ctx.sync()
                ms[k].append((time.perf_counter() - t0) / steps * 1e3)
        return {k: {"ms": v, "median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "steps": legs[k][1]}
                for k, v in ms.items()}

    result = {"commit": a.commit, "warmup": a.warmup, "repeat": a.repeat,
              "timing": "host clock around synchronous calls, mean per call over `steps` calls; legs alternate per repeat",
              "clusters": {}}
    for config in [int(x) for x in a.configs.split(",")]:
        cfg, nodes, pods = synth.cluster(config)
        batch = engine.PodBatch(ctx, pods)
        snap = engine.Snapshot(ctx, cfg.kg_config(), nodes)
        cases = {}
        for n_rows in [int(x) for x in a.rows.split(",")]:
            n_rows = min(n_rows, batch.n)
            # evenly spread batch positions; all rows: None (every pod in batch order)
            rows = None if n_rows == batch.n else (np.arange(n_rows, dtype=np.uint64) * batch.n // n_rows).astype(np.uint32)
            pairs = n_rows * snap.n
            steps = int(max(1, min(a.max_steps, a.pairs_per_window // pairs)))
            vsteps = int(max(1, min(a.max_steps, a.verify_pairs_per_window // pairs)))
            r = {"n_rows": n_rows, "pairs": pairs, "bitmap_bytes": n_rows * nodesets.words(snap.n) * 4}

            def feasible(name):
                def run():
                    form(name)
                    return engine.eval_feasible(snap, batch, rows)
                return run

            legs = {"feasible_rows": (feasible("rows"), steps), "feasible_records": (feasible("records"), steps),
                    "feasible_default": (feasible(None), steps),
                    "diagnose": (lambda: engine.eval_diagnose(snap, batch, rows, first_plugin=False), steps)}
            by_rows, by_records = feasible("rows")(), feasible("records")()
            r["forms_equal"] = bool(np.array_equal(by_rows, by_records))
            sub = None
            if pairs <= a.verify_pairs:
                sub = batch if rows is None else engine.PodBatch(ctx, abi.take(pods, rows.astype(np.int64)))
                st = status_only(snap, sub)
                r["equal_verify_route"] = bool(np.array_equal(by_rows, nodesets.pack(st == 0)))
                r["feasible_share"] = float((st == 0).mean())
                del st
                legs["verify_status"] = (lambda: status_only(snap, sub), vsteps)
                r["verify_matrix_bytes"] = pairs * 4
                r["verify_device_bytes"] = pairs * 37
            else:
                r["verify_status"] = f"not measured: {pairs} pairs, a status matrix of {pairs * 4 / 1e9:.1f} GB on the " \
                                     f"host and {pairs * 37 / 1e9:.1f} GB of device buffers"
            r.update(timed(legs))
            form(None)
            if sub is not None and sub is not batch:
                sub.close()
            cases[str(n_rows)] = r
            print(f"config{config} rows={n_rows}: " + ", ".join(
                f"{k}={v['median_ms']:.3f}" for k, v in r.items() if isinstance(v, dict)), file=sys.stderr, flush=True)
        result["clusters"][f"config{config}"] = {"n_nodes": snap.n, "n_pods": batch.n, "rows": cases}
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
