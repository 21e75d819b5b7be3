#!/usr/bin/env python3
"""A/B aid for the per-pod host score terms, on bench config 2's nodes and pods under bench.py's warm-up and step
counts, profiling off (host clock around `steps` asynchronous selects and one sync). It imports the package of the tree
it lies in.

Cases (ms per top-1 select):
  none           no terms: the step bench.py measures (the one-pod-block select)
  none_general   no terms, KG_NO_SMALL_SELECT=1: the general path, the kernel shape the term lanes replace
  a_raw1         one shared RAW row for every pod
  b_norm8        every pod carries one of 8 NORMALIZE rows
  c_tenth        one pod in ten carries a row of b_norm8: what leaving the one-pod-block select costs
  d_norm8_sets8  b_norm8 together with one of 8 random half-cluster candidate node sets per pod

Each case with terms is also measured the way a caller has to do it without them (`host_*` fields): kg_eval_verify with
only the total matrix downloaded (an infeasible pair's total is -1), the terms added and the argmax taken with numpy on
the host, once per repeat. That route's keys are compared with the device's for every pod; a difference ends the run.

    python tools/node_scores_ab.py [--steps 20] [--warmup 3] [--repeat 3] [--no-host]

Prints one JSON line per (case, repeat)."""
import argparse
import ctypes as C
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
    ap.add_argument("--no-host", action="store_true", help="skip the verify + host argmax route")
    a = ap.parse_args()

    import numpy as np

    from koordinator_amd import abi, engine, nodescores, nodesets, synth

    cfg, nodes, pods = synth.cluster(2)
    n, p = abi.table_len(nodes), abi.table_len(pods)
    ctx = engine.Context(0)
    snap = engine.Snapshot(ctx, cfg.kg_config(), nodes)
    batch = engine.PodBatch(ctx, pods)
    rng = np.random.default_rng(2)

    def time_select():
        for _ in range(a.warmup):
            engine.eval_select_async(snap, batch, 1)
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            engine.eval_select_async(snap, batch, 1)
        ctx.sync()
        return (time.perf_counter() - t0) / a.steps * 1e3

    total = np.zeros((p, n), np.int64)

    def host_route(pod_terms, raw, mode, weight, mask):
        """(verify ms, host ms, keys): today's route for the same pods, on a batch without terms."""
        plain = engine.PodBatch(ctx, pods)
        if mask is not None:
            plain.set_node_sets(*mask, n)
        out = abi.KgVerifyOut()
        out.total = total.ctypes.data_as(C.POINTER(C.c_int64))
        t0 = time.perf_counter()
        ctx.check(ctx.L.kg_eval_verify(snap.h, plain.h, C.byref(out)), "kg_eval_verify")
        t1 = time.perf_counter()
        ok = total >= 0
        tot = total.copy()
        for r in np.unique(pod_terms[pod_terms >= 0]):
            who = np.flatnonzero((pod_terms == r).any(axis=1))
            row = raw[r].astype(np.int64)
            if mode[r] == abi.KG_SCORE_RAW:
                val = np.broadcast_to(row, (len(who), n))
            else:
                m = np.where(ok[who], row[None, :], 0).max(axis=1)[:, None]
                q = 100 * row[None, :] // np.maximum(m, 1)
                if mode[r] == abi.KG_SCORE_NORMALIZE_REVERSE:
                    val = np.where(m == 0, 100, 100 - q)
                else:
                    val = np.where(m == 0, 0, q)
            tot[who] += np.where(ok[who], int(weight[r]) * val, 0)
        best = tot.argmax(axis=1)  # the first of equal totals: the lowest snapshot index
        bt = tot[np.arange(p), best]
        keys = np.where(bt >= 0, (bt.astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - best.astype(np.uint64)),
                        np.uint64(0))
        t2 = time.perf_counter()
        plain.close()
        return (t1 - t0) * 1e3, (t2 - t1) * 1e3, keys

    def terms_of(case):
        if case == "a_raw1":
            lists = [[(rng.integers(0, 101, n), abi.KG_SCORE_RAW, 1)]] * p
        else:
            rows = [rng.integers(0, 1001, n) for _ in range(8)]
            pick = rng.integers(0, 8, p)
            lists = [[(rows[pick[j]], abi.KG_SCORE_NORMALIZE, 2)] if case != "c_tenth" or j % 10 == 0 else None
                     for j in range(p)]
        return nodescores.from_terms(lists, n)

    for case in ("none", "none_general", "a_raw1", "b_norm8", "c_tenth", "d_norm8_sets8"):
        env = {"KG_NO_SMALL_SELECT": "1"} if case == "none_general" else {}
        terms = mask = None
        batch.clear_node_scores()
        batch.clear_node_sets()
        if not case.startswith("none"):
            terms = terms_of(case)
            batch.set_node_scores(*terms, n)
        if case == "d_norm8_sets8":
            mask = (rng.integers(0, 8, p).astype(np.int32), nodesets.pack(rng.random((8, n)) < 0.5))
            batch.set_node_sets(*mask, n)
        os.environ.update(env)
        lanes = batch.select_lanes()[0]
        for rep in range(a.repeat):
            line = {"case": case, "pods": p, "nodes": n, "lanes": lanes, "repeat": rep, "steps": a.steps,
                    "warmup": a.warmup, "select_ms_per_step": time_select()}
            if terms is not None and not a.no_host:
                keys = engine.result_keys(batch, 1)[:, 0]
                vms, hms, want = host_route(*terms, mask)
                if not np.array_equal(keys, want):
                    raise SystemExit(f"{case}: the device's keys differ from verify + host argmax "
                                     f"({int((keys != want).sum())} pods)")
                line.update(host_verify_total_ms=vms, host_argmax_ms=hms, keys_equal=True)
            print(json.dumps(line), flush=True)
        for k in env:
            del os.environ[k]
    batch.close()
    snap.close()
    ctx.close()


if __name__ == "__main__":
    main()
