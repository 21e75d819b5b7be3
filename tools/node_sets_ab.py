#!/usr/bin/env python3
"""A/B aid for the per-pod candidate node sets, on bench config 2's nodes and pods under bench.py's warm-up and step
counts, profiling off (host clock around `steps` asynchronous selects and one sync). It imports the package of the tree
it lies in, so copy it into the tree to be measured (as tools/dedup_ab.py); in a tree without PodBatch.set_node_sets it
runs the cases without sets only.

Cases (ms per top-1 select):
  none           no sets: the step bench.py measures (the one-pod-block select)
  none_general   no sets, KG_NO_SMALL_SELECT=1: the general path, the kernel shape the set lanes replace
  a_half8        every pod carries one of 8 random half-cluster sets
  b_pool64       every pod carries one of 64 sets of 16 nodes: the block skip must put it below a_half8
  c_tenth        one pod in ten carries a set of a_half8: what leaving the one-pod-block select costs

    python tools/node_sets_ab.py [--steps 20] [--warmup 3] [--repeat 3] [--check]

--check compares every case's keys with the unmasked select restricted by hand (sampled pods, host arithmetic on the
verify matrix of those pods). Prints one JSON line per (case, repeat)."""
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
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()

    import numpy as np

    from koordinator_amd import abi, engine, synth

    have_sets = hasattr(engine.PodBatch, "set_node_sets")
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

    def masks(case):
        """(pod_set, set masks bool[S, N]) of a case"""
        if case in ("a_half8", "c_tenth"):
            sets = rng.random((8, n)) < 0.5
            pod_set = rng.integers(0, 8, p).astype(np.int32)
            if case == "c_tenth":
                pod_set[np.arange(p) % 10 != 0] = -1
            return pod_set, sets
        sets = np.zeros((64, n), bool)
        for s in range(64):
            sets[s, rng.choice(n, 16, replace=False)] = True
        return rng.integers(0, 64, p).astype(np.int32), sets

    def check(case, pod_set, sets):
        keys = engine.result_keys(batch, 1)[:, 0]
        sample = np.concatenate([np.arange(0, p, 97), np.flatnonzero(pod_set >= 0)[:40]])
        sub = engine.PodBatch(ctx, abi.take(pods, sample))
        ver = engine.eval_verify(snap, sub)
        sub.close()
        node = np.uint64(0xFFFFFFFF) - np.arange(n, dtype=np.uint64)
        allk = ((ver.total & 0xFFFFFFFF).astype(np.uint64) << np.uint64(32)) | node[None, :]
        ok = ver.status == 0
        for t, j in enumerate(sample):
            if pod_set[j] >= 0:
                ok[t] &= sets[pod_set[j]]
        want = np.where(ok, allk, np.uint64(0)).max(axis=1)
        if not np.array_equal(keys[sample], want):
            raise SystemExit(f"{case}: keys differ from the restricted verify matrix")

    cases = ["none", "none_general"] + (["a_half8", "b_pool64", "c_tenth"] if have_sets else [])
    for case in cases:
        env = {}
        pod_set = sets = None
        if case == "none_general":
            env["KG_NO_SMALL_SELECT"] = "1"
        if case in ("a_half8", "b_pool64", "c_tenth"):
            from koordinator_amd import nodesets
            pod_set, sets = masks(case)
            batch.set_node_sets(pod_set, nodesets.pack(sets), n)
        elif have_sets:
            batch.clear_node_sets()
        os.environ.update(env)
        lanes = batch.select_lanes()[0] if hasattr(batch, "select_lanes") else p
        for rep in range(a.repeat):
            ms = time_select()
            print(json.dumps({"build": "sets" if have_sets else "parent", "case": case, "pods": p, "nodes": n,
                              "lanes": lanes, "repeat": rep, "steps": a.steps, "warmup": a.warmup,
                              "select_ms_per_step": ms}), flush=True)
        if a.check and pod_set is not None:
            check(case, pod_set, sets)
        for k in env:
            del os.environ[k]
    batch.close()
    snap.close()
    ctx.close()


if __name__ == "__main__":
    main()
