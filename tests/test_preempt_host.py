"""Host side of the preemption dry run (no device): include/koordgpu.h against abi.py, build_residents and the importance
order, the PDB matching and split and the potential-victim rule against koord-scheduler's test tables
(tests/golden/preempt_pdb_kat.json, values only), pick_one_node on hand-made summaries, and the vectorised reference
(preempt_ref.preempt) against its scalar per-node restatement."""
import ctypes as C
import json
import os
import re

import numpy as np

import preempt_ref as ref
from koordinator_amd import abi, preempt, synth
from koordinator_amd.config import SchedulerConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "koordgpu.h")
KAT = json.load(open(os.path.join(ROOT, "tests", "golden", "preempt_pdb_kat.json")))
GI = 1 << 30
RESULT = {"CANDIDATE": abi.KG_PREEMPT_CANDIDATE, "NO_VICTIMS": abi.KG_PREEMPT_NO_VICTIMS}


def make_pod(name, priority=None, quota=None, cpu=0, mem=0, ns="default", labels=None, start=None, preemptible_label=None,
             disable_preemptible=None, annotations=None):
    labels = dict(labels or {})
    if quota is not None:
        labels[preempt.LABEL_QUOTA_NAME] = quota
    if preemptible_label is not None:
        labels[preempt.LABEL_QUOTA_PREEMPTIBLE] = preemptible_label
    if disable_preemptible is not None:
        labels[preempt.LABEL_DISABLE_PREEMPTIBLE] = disable_preemptible
    req = {}
    if cpu:
        req["cpu"] = f"{cpu}m"
    if mem:
        req["memory"] = str(mem)
    pod = {"metadata": {"name": name, "namespace": ns, "labels": labels, "annotations": annotations or {}},
           "spec": {"containers": [{"name": "c", "resources": {"requests": req}}]}, "status": {}}
    if priority is not None:
        pod["spec"]["priority"] = priority
    if start is not None:
        pod["status"]["startTime"] = start
    return pod


# ---- the header and its mirror -----------------------------------------------------------------------------------
def test_header_constants_and_structs_match_abi(tmp_path):
    src = open(HEADER).read()
    for name in ("KG_RES_MAX_PER_NODE", "KG_RES_PDBS", "KG_RES_NON_PREEMPTIBLE", "KG_RES_NUMA_ALLOC", "KG_RES_PDB_OVERFLOW",
                 "KG_PREEMPT_SKIP_NON_PREEMPTIBLE", "KG_PREEMPT_SAME_GROUP", "KG_PREEMPT_CANDIDATE", "KG_PREEMPT_NO_VICTIMS",
                 "KG_PREEMPT_NO_FIT", "KG_PREEMPT_UNSUPPORTED", "KG_PREEMPT_EXCLUDED"):
        m = re.search(rf"^#define {name}\s+(0x[0-9a-fA-F]+|\d+)u?\b", src, re.M)
        assert m, f"{name} is not defined in include/koordgpu.h"
        assert int(m.group(1), 0) == getattr(abi, name), name
    assert abi.KG_PREEMPT_MASK_WORDS * 32 == abi.KG_RES_MAX_PER_NODE
    for fn in ("kg_snapshot_upload_residents", "kg_snapshot_update_residents", "kg_snapshot_read_residents", "kg_eval_preempt"):
        assert re.search(rf"^kg_status {fn}\(", src, re.M), fn
    assert "new within ABI 14" in src[src.index("KG_PREEMPT_EXCLUDED"):src.index("kg_status kg_eval_preempt(")]
    import subprocess
    prog = tmp_path / "sz.c"
    prog.write_text(f'#include "{HEADER}"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){{'
                    'printf("%zu %zu %zu %zu %zu\\n", sizeof(kg_preempt_node), sizeof(kg_resident_columns), '
                    'offsetof(kg_preempt_node, top_priority), offsetof(kg_preempt_node, sum_priority), '
                    'offsetof(kg_resident_columns, req_cpu));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", str(prog), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert sizes == [C.sizeof(abi.KgPreemptNode), C.sizeof(abi.KgResidentColumns), abi.KgPreemptNode.top_priority.offset,
                     abi.KgPreemptNode.sum_priority.offset, abi.KgResidentColumns.req_cpu.offset]
    assert sizes[0] == 32 == abi.PREEMPT_NODE_DTYPE.itemsize
    for f in abi.PREEMPT_NODE_DTYPE.names:
        assert abi.PREEMPT_NODE_DTYPE.fields[f][1] == getattr(abi.KgPreemptNode, f).offset, f


def test_library_exports_the_calls():
    from koordinator_amd import engine
    L = engine.lib()
    assert L.kg_eval_preempt.argtypes[-2] == C.POINTER(abi.KgPreemptNode)
    assert len(L.kg_eval_preempt.argtypes) == 11 and len(L.kg_snapshot_update_residents.argtypes) == 5
    assert hasattr(L, "kg_snapshot_read_residents") and hasattr(L, "kg_snapshot_upload_residents")


# ---- build_residents ---------------------------------------------------------------------------------------------
def test_build_residents_and_importance_order():
    pdbs = [
        {"metadata": {"namespace": "default"}, "spec": {"selector": {"matchLabels": {"app": "a"}}}, "status": {"disruptionsAllowed": 1}},
        {"metadata": {"namespace": "default"}, "spec": {"selector": {"matchExpressions": [{"key": "tier", "operator": "Exists"}]}},
         "status": {"disruptionsAllowed": 0, "disruptedPods": {"p3": "2024-01-01T00:00:00Z"}}},
        {"metadata": {"namespace": "default"}, "spec": {"selector": {"matchLabels": {"app": "a"}}}, "status": {"disruptionsAllowed": 2}},
        {"metadata": {"namespace": "default"}, "spec": {"selector": {"matchExpressions": [{"key": "app", "operator": "In", "values": ["a", "b"]}]}},
         "status": {}},
    ]
    status = json.dumps({"cpuset": "0-3"})
    node0 = [
        make_pod("p0", 100, "q1", 500, GI, labels={"app": "a"}, start="2024-05-01T10:00:00Z"),            # pdb 0, 2, 3: overflow
        make_pod("p1", 9000, "q2", 1000, 2 * GI, start="2024-05-01T09:00:00Z", preemptible_label="false"),
        make_pod("p2", 100, None, 250, 0, labels={"tier": "x"}, start="2024-05-01T08:00:00Z"),           # pdb 1; default quota
        make_pod("p3", None, "q1", 0, 0, labels={"tier": "x"}),                                           # in pdb 1's DisruptedPods
    ]
    node2 = [make_pod("p4", 5000, "q1", 4000, 8 * GI, labels={"app": "b"}, start=1_700_000_000,
                      annotations={preempt.ANN_RESOURCE_STATUS: status})]
    t, groups = preempt.build_residents([node0, [], node2], pdbs, now=1_800_000_000)
    assert abi.table_len(t) == 5 and list(t["node"]) == [0, 0, 0, 0, 2]
    assert list(t["priority"]) == [100, 9000, 100, 0, 5000]
    assert t["start_time"][0] == 1714557600 and t["start_time"][3] == 1_800_000_000 and t["start_time"][4] == 1_700_000_000
    assert groups == {"q1": 0, "q2": 1, preempt.DEFAULT_QUOTA_NAME: 2} and list(t["group"]) == [0, 1, 2, 0, 0]
    NP, NA, OV = abi.KG_RES_NON_PREEMPTIBLE, abi.KG_RES_NUMA_ALLOC, abi.KG_RES_PDB_OVERFLOW
    assert list(t["flags"]) == [OV, NP, NP, 0, NA]  # p2: the default quota is shielded
    assert list(t["pdb0"]) == [0, -1, 1, -1, 3] and list(t["pdb1"]) == [2, -1, -1, -1, -1]
    assert list(t["req_cpu"]) == [500, 1000, 250, 0, 4000] and list(t["req_mem"]) == [GI, 2 * GI, 0, 0, 8 * GI]
    assert list(t["nz_cpu"]) == [500, 1000, 250, 100, 4000], "NonZeroRequested: the default 100m of a pod without a request"
    assert list(preempt.pdb_allowed(pdbs)) == [1, 0, 2, 0]
    # the reservation plugin: its own label, no group, the default quota not shielded
    t2, g2 = preempt.build_residents([[make_pod("r0", 5, None, disable_preemptible="true"), make_pod("r1", 5, None, preemptible_label="false")]],
                                     plugin=preempt.RESERVATION)
    assert list(t2["flags"]) == [NP, 0] and list(t2["group"]) == [-1, -1] and g2 == {}
    # importance: higher priority first, then earlier start, ties in input order; preempt_ref.node_lists is the same order
    order = preempt.importance_order(t["priority"][:4], t["start_time"][:4])
    assert list(order) == [1, 2, 0, 3]
    assert [list(l) for l in ref.node_lists(t, 3)] == [[1, 2, 0, 3], [], [4]]
    tie = preempt.importance_order([5, 5, 7, 5], [10, 10, 99, 10])
    assert list(tie) == [2, 0, 1, 3]


# ---- the reference's tables --------------------------------------------------------------------------------------
def test_pdb_matching_and_split_against_the_reference_tables():
    assert len(KAT["pdb"]) == 14
    for case in KAT["pdb"]:
        budgets = [preempt.matching_pdbs(p, case["pdbs"]) for p in case["pods"]]
        viol, ok = preempt.split_pdb_violation(budgets, preempt.pdb_allowed(case["pdbs"]))
        assert (len(viol), len(ok)) == (case["want_violating"], case["want_non_violating"]), case["name"]
        assert viol == sorted(viol) and ok == sorted(ok), "the order inside both groups is kept"
        if "want_violating_names" in case:
            assert [case["pods"][k]["metadata"]["name"] for k in viol] == case["want_violating_names"], case["name"]
        # the same through the table and the vectorised split of the reference loop
        t, _ = preempt.build_residents([case["pods"]], case["pdbs"])
        cols = {k: v[None, :] for k, v in t.items()}
        if abi.table_len(t):
            v2 = ref.violating(cols, np.ones((1, abi.table_len(t)), bool), preempt.pdb_allowed(case["pdbs"]))
            assert list(np.flatnonzero(v2[0])) == viol, case["name"]


def test_can_preempt_table_against_the_potential_victim_rule():
    both = abi.KG_PREEMPT_SKIP_NON_PREEMPTIBLE | abi.KG_PREEMPT_SAME_GROUP
    cases = KAT["can_preempt"]["cases"]
    assert len(cases) == 6 and sum(c["want"] for c in cases) == 1
    for case in cases:
        v, p = case["victim"], case["preemptor"]
        t, groups = preempt.build_residents([[make_pod("victim", v["priority"], v["quota"], 1000, GI,
                                                       preemptible_label=v.get("preemptible_label"))]])
        pg = groups.get(p["quota"] or preempt.DEFAULT_QUOTA_NAME, -1)
        got = preempt.can_preempt(p["priority"], pg, int(t["priority"][0]), int(t["group"][0]), int(t["flags"][0]), both)
        assert got == case["want"], case["name"]
        cols = {k: a[None, :] for k, a in t.items()}
        assert bool(ref.potential(cols, np.ones((1, 1), bool), p["priority"], pg, both)[0, 0]) == case["want"], case["name"]


def test_select_victims_tables_with_the_plain_plugins():
    """The reference's SelectVictimsOnNode cases that need only the plain plugins. All four end with 0 victims (the two
    that produce or reprieve a victim are skipped, reasons in the JSON), so they pin the potential-victim rule and the
    all-reprieved outcome; real victims through scalar_node come from the generated clusters (the n33 test below)."""
    sel = KAT["select_victims"]
    assert len(sel["cases"]) == 4 and len(sel["skipped"]) == 2 and all(s["reason"] for s in sel["skipped"])
    assert all(case["want_victims"] == 0 for case in sel["cases"]) and "0 victims" in sel["coverage"]
    cfg = SchedulerConfig(plugins=abi.KG_PLUGIN_NRF)
    kc = cfg.kg_config()
    for case in sel["cases"]:
        plugin = case["plugin"]
        flags = abi.KG_PREEMPT_SKIP_NON_PREEMPTIBLE | (abi.KG_PREEMPT_SAME_GROUP if plugin == preempt.ELASTIC_QUOTA else 0)
        running = [make_pod(p["name"], p["priority"], p["quota"], p["cpu"], p["mem"], preemptible_label=p.get("preemptible_label"),
                            start=1_700_000_000 + k) for k, p in enumerate(case["pods"])]
        res, groups = preempt.build_residents([running], plugin=plugin, cfg=cfg)
        nodes = abi.empty_nodes(1)
        for k in ("alloc_cpu", "alloc_mem", "alloc_pods"):
            nodes[k][0] = case["node"][k]
        for col in ref.MOVE_COLUMNS:
            nodes[col][0] = res[col].sum()
        nodes["num_pods"][0] = len(running)
        nodes["cpu_amp_ratio"][0] = 1.0
        p = case["preemptor"]
        pods = abi.empty_pods(1)
        pods["req_cpu"][0] = pods["nz_cpu"][0] = p["cpu"]
        pods["req_mem"][0] = p["mem"]
        pods["nz_mem"][0] = p["mem"] or 200 * (1 << 20)
        pods["flags"][0] = (abi.KG_POD_HAS_CPU if p["cpu"] else 0) | (abi.KG_POD_HAS_MEM if p["mem"] else 0)
        pg = groups.get(p["quota"], -1) if p["quota"] else -1
        r, st, victims, n_viol, n_pot = ref.scalar_node(kc, nodes, pods, res, 0, 0, p["priority"], pg, allowed=[], flags=flags)
        assert (r, len(victims), n_viol) == (RESULT[case["want_result"]], case["want_victims"], case["want_violating"]), case["name"]
        out, vic = ref.preempt(kc, nodes, pods, res, [0], [p["priority"]], [pg], allowed=np.zeros(0, np.int32), flags=flags)
        assert (out["result"][0, 0], out["n_victims"][0, 0], out["n_violating"][0, 0]) == (r, len(victims), n_viol), case["name"]


# ---- pick_one_node -----------------------------------------------------------------------------------------------
def summary(*nodes):
    s = np.zeros(len(nodes), abi.PREEMPT_NODE_DTYPE)
    for i, n in enumerate(nodes):
        for k, v in n.items():
            s[k][i] = v
    return s


def cand(n_victims=1, n_violating=0, top_priority=100, sum_priority=None, top_start=1000):
    return dict(result=abi.KG_PREEMPT_CANDIDATE, n_victims=n_victims, n_violating=n_violating, top_priority=top_priority,
                sum_priority=top_priority * n_victims if sum_priority is None else sum_priority, top_start=top_start)


def test_pick_one_node_one_summary_per_criterion():
    pick = preempt.pick_one_node
    assert pick(summary()) == -1
    assert pick(summary(dict(result=abi.KG_PREEMPT_NO_FIT), dict(result=abi.KG_PREEMPT_NO_VICTIMS),
                        dict(result=abi.KG_PREEMPT_UNSUPPORTED), dict(result=abi.KG_PREEMPT_EXCLUDED))) == -1
    assert pick(summary(cand(n_victims=0), dict(result=abi.KG_PREEMPT_NO_FIT))) == -1, "a candidate without victims needs no preemption"
    # 1. fewest violations, before everything else
    assert pick(summary(cand(1, 1, top_priority=0), cand(3, 0, top_priority=9000))) == 1
    # 2. lowest highest victim priority
    assert pick(summary(cand(1, 0, 500), cand(4, 0, 400, sum_priority=1600))) == 1
    # 3. lowest sum of priority + 2^31: one victim of -10 beats two of -10 and -2000000000 although the plain sum is lower
    assert pick(summary(cand(2, 0, -10, sum_priority=-2000000010), cand(1, 0, -10, sum_priority=-10))) == 1
    assert pick(summary(cand(2, 0, 100, sum_priority=200), cand(2, 0, 100, sum_priority=150))) == 1
    # 4. fewest victims: a victim of priority -2^31 adds nothing to the shifted sum, so both sums are 100 + 2^31 and the
    # top priorities are equal; only the victim count differs
    assert pick(summary(cand(2, 0, 100, sum_priority=100 - 2**31), cand(1, 0, 100, sum_priority=100))) == 1
    # 5. latest start of the top victims
    assert pick(summary(cand(1, 0, 100, top_start=1000), cand(1, 0, 100, top_start=2000), cand(1, 0, 100, top_start=1500))) == 1
    # 6. lowest index
    assert pick(summary(dict(result=abi.KG_PREEMPT_NO_FIT), cand(), cand())) == 1
    # non-candidates never win on their (zero) fields
    assert pick(summary(dict(result=abi.KG_PREEMPT_UNSUPPORTED, n_victims=1), cand(2, 1, 9000))) == 1


# ---- the reference against its scalar restatement ------------------------------------------------------------------
def test_vectorised_reference_equals_the_scalar_loop_on_n33():
    c = ref.case_inputs("n33", synth)
    seen = set()
    for flags in (0, abi.KG_PREEMPT_SKIP_NON_PREEMPTIBLE, abi.KG_PREEMPT_SKIP_NON_PREEMPTIBLE | abi.KG_PREEMPT_SAME_GROUP):
        out, vic = ref.preempt(c["kc"], c["nodes"], c["pods"], c["res"], c["rows"], c["priority"], c["group"], flags=flags)
        for t, j in enumerate(c["rows"]):
            for i in range(abi.table_len(c["nodes"])):
                r, st, victims, n_viol, n_pot = ref.scalar_node(c["kc"], c["nodes"], c["pods"], c["res"], i, int(j),
                                                                int(c["priority"][t]), int(c["group"][t]), flags=flags)
                o = out[t, i]
                assert (r, st, len(victims), n_viol, n_pot) == (o["result"], o["status"], o["n_victims"], o["n_violating"],
                                                                o["n_potential"]), (flags, t, i)
                assert sorted(victims) == list(preempt.victim_positions(vic[t, i])), (flags, t, i)
                if victims:
                    lst = ref.node_lists(c["res"], 33)[i]
                    pr = c["res"]["priority"][lst[victims]]
                    assert o["sum_priority"] == pr.sum() and o["top_priority"] == pr.max()
                    assert o["top_start"] == c["res"]["start_time"][lst[victims]][pr == pr.max()].min()
                seen.add(int(r))
    assert seen >= {abi.KG_PREEMPT_CANDIDATE, abi.KG_PREEMPT_NO_VICTIMS, abi.KG_PREEMPT_NO_FIT, abi.KG_PREEMPT_UNSUPPORTED}
