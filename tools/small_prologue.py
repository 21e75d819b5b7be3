#!/usr/bin/env python3
"""The prologue of config 2's one-launch select: per workgroup, from entry to "pod operands ready" (thread 0's clock behind
order[j], load_pod and to_podf), from the PH aid's phase file and its .ops companion. One JSON line per run."""
import json
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from koordinator_amd import engine, synth

cfg, nodes, pods = synth.cluster(2)
ctx = engine.Context(0)
snap = engine.Snapshot(ctx, cfg.kg_config(), nodes)
batch = engine.PodBatch(ctx, pods)
for run in range(3):
    for _ in range(3):
        engine.eval_select_async(snap, batch, 1)
    ctx.sync()
    fd, path = tempfile.mkstemp(suffix=".phases")
    os.close(fd)
    os.environ["KG_SMALL_PHASES"] = path
    for _ in range(20):
        engine.eval_select_async(snap, batch, 1)
    ctx.sync()
    del os.environ["KG_SMALL_PHASES"]
    raw = np.fromfile(path, dtype=np.uint64)
    ops = np.fromfile(path + ".ops", dtype=np.uint64)
    os.remove(path)
    os.remove(path + ".ops")
    per, at, at2 = [], 0, 0
    while at < len(raw):
        nc = int(raw[at])
        t = raw[at + 1:at + 1 + 4 * nc].reshape(nc, 4).astype(np.int64)
        assert int(ops[at2]) == nc
        o = ops[at2 + 1:at2 + 1 + nc].astype(np.int64)
        at += 1 + 4 * nc
        at2 += 1 + nc
        pro = o - t[:, 0]
        last = int(np.argmax(t[:, 1]))  # the workgroup whose loops end last
        per.append((np.median(pro), pro.max(), pro[last], np.median(t[:, 1] - t[:, 0]), (t[:, 1] - t[:, 0])[last],
                    np.median(pro[t[:, 0] - t[:, 0].min() < 20]), nc))
    m = np.median(np.array(per, dtype=np.float64), axis=0)
    print(json.dumps({"nodes": "config2", "run": run + 1, "launches": len(per), "workgroups": int(m[6]),
                      "prologue_median_us": m[0] / 100.0, "prologue_max_us": m[1] / 100.0,
                      "prologue_of_last_workgroup_us": m[2] / 100.0, "loops_own_median_us": m[3] / 100.0,
                      "loops_own_of_last_workgroup_us": m[4] / 100.0,
                      "prologue_median_of_workgroups_entering_in_first_0.2us": m[5] / 100.0,
                      "unit": "us of the 100 MHz device clock, medians over 20 launches; prologue = thread 0's entry to "
                              "its lane's PodF converted (order[j], load_pod, to_podf); last workgroup = the one whose loops end last"}), flush=True)
