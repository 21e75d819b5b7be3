#!/usr/bin/env python3
"""Cost of the FitError diagnosis (kg_eval_diagnose) against the only other way to the same counts: kg_eval_verify of
the pods in question with only the status matrix requested, plus a histogram of it on the host. It imports the package
of the tree it lies in and needs an MI355X.

Timed, each as the mean of --steps synchronous calls after --warmup, --repeat times (host clock; every call ends in a
stream synchronise):
  diagnose_all      eval_diagnose of every pod of config 2 (10k pods x 10k nodes)
  diagnose_100      eval_diagnose of 100 rows of the same batch (the pods the select left without a node first)
  verify_100        eval_verify (status only) of a batch holding just those 100 pods: kernel + download of the matrix;
                    uploading that batch (upload_100) and the numpy histogram of the matrix (histogram_100, 32 passes
                    over it; a compiled one would be faster) are timed apart and are NOT part of verify_100
on config 2's cluster and, for the 100-row legs, on config 4's (100k nodes). The counts of the two routes are compared
once per cluster.

    python tools/diagnose_rate.py [--steps 20] [--warmup 3] [--repeat 3] [--commit ID] [--out FILE]

Prints one JSON object and writes it to --out (default profiles/diagnose/diagnose_rate.json)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--rows", type=int, default=100)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diagnose", "diagnose_rate.json"))
    a = ap.parse_args()

    import numpy as np

    from koordinator_amd import abi, engine, synth

    ctx = engine.Context(0)

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        ctx.sync()
        out = []
        for _ in range(a.repeat):
            t0 = time.perf_counter()
            for _ in range(a.steps):
                fn()
            ctx.sync()
            out.append((time.perf_counter() - t0) / a.steps * 1e3)
        return {"ms": out, "median_ms": statistics.median(out)}

    def status_only(snap, batch):
        st = np.zeros((batch.n, snap.n), np.uint32)
        out = abi.KgVerifyOut()
        out.status = st.ctypes.data_as(C.POINTER(C.c_uint32))
        snap.ctx.check(snap.ctx.L.kg_eval_verify(snap.h, batch.h, C.byref(out)), "kg_eval_verify")
        return st

    def histogram(st):
        out = np.zeros((st.shape[0], abi.KG_DIAG_SLOTS), np.uint32)
        for b in range(32):
            out[:, b] = ((st >> np.uint32(b)) & np.uint32(1)).sum(axis=1)
        code = ((st >> np.uint32(24)) & np.uint32(3)) | (((st >> np.uint32(6)) & np.uint32(3)) << np.uint32(2))
        for c in range(1, 16):
            out[:, abi.KG_DIAG_DEV_CODE0 + c] = (code == c).sum(axis=1)
        out[:, abi.KG_DIAG_FEASIBLE] = (st == 0).sum(axis=1)
        return out

    result = {"commit": a.commit, "steps": a.steps, "warmup": a.warmup, "repeat": a.repeat, "rows": a.rows,
              "timing": "host clock around synchronous calls, mean per call", "clusters": {}}
    for name, config in (("config2", 2), ("config4", 4)):
        cfg, nodes, pods = synth.cluster(config)
        batch = engine.PodBatch(ctx, pods)
        snap = engine.Snapshot(ctx, cfg.kg_config(), nodes)
        keys = engine.eval_select(snap, batch, 1)[:, 0]
        failed = np.flatnonzero(keys == 0)
        rows = np.concatenate([failed, np.flatnonzero(keys != 0)])[:a.rows].astype(np.uint32)
        sub = engine.PodBatch(ctx, abi.take(pods, rows))
        # the two routes give the same counts (all bits: what the verify matrix holds)
        same = bool(np.array_equal(engine.eval_diagnose(snap, batch, rows=rows, first_plugin=False),
                                   histogram(status_only(snap, sub))))
        r = {"n_nodes": snap.n, "n_pods": batch.n, "unschedulable_pods": int(len(failed)),
             "unschedulable_among_rows": int(min(len(failed), a.rows)), "counts_equal_verify_route": same}
        if name == "config2":
            r["diagnose_all"] = timed(lambda: engine.eval_diagnose(snap, batch))
        r["diagnose_100"] = timed(lambda: engine.eval_diagnose(snap, batch, rows=rows))
        r["verify_100"] = timed(lambda: status_only(snap, sub))
        r["verify_100_matrix_bytes"] = int(len(rows)) * snap.n * 4
        r["verify_100_device_bytes"] = int(len(rows)) * snap.n * 37
        sub_pods = abi.take(pods, rows)
        r["upload_100"] = timed(lambda: sub.upload(sub_pods))
        st = status_only(snap, sub)
        t0 = time.perf_counter()
        histogram(st)
        r["histogram_100_numpy_ms"] = (time.perf_counter() - t0) * 1e3
        result["clusters"][name] = r
        sub.close()
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
