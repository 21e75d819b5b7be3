"""kg_eval_offer_slots on the device: per node, how many of a job's pods fit when they are added one after another
(calculateNodeOfferSlot, coscheduling/core/network_topology_solver.go:113-158), and the status word of the first pod
that does not, against the loop rebuilt from the CPU oracle (offer_slots_ref).

Bar: exact (np.array_equal) on both outputs. The inputs are shown, from the reference alone, to tell the loop from its
two wrong readings: counts without accumulation, and counts with the whole Reserve between pods. Measured on the CPU
(first 48 pods in order; nodes whose count differs from no accumulation / from the full Assume):
  small 117 / 81   small_x4 12 / 12   mixed 116 / 75   n129 38 / 75"""
import ctypes as C
import functools

import numpy as np
import pytest

import node_scores_ref
import node_sets_ref as sets_ref
import offer_slots_ref as ref
import oracle_lib
from koordinator_amd import abi, batch, engine, synth

pytestmark = pytest.mark.gpu

EXCL = abi.KG_ST_NODE_EXCLUDED
DISCRIMINATING = ("small", "small_x4", "mixed", "n129")


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def case(name):
    """(kg_config, nodes, pods) of one cluster; read-only."""
    cfg, nodes, pods = ref.CLUSTERS[name](synth)
    return cfg.kg_config(), nodes, pods


@functools.lru_cache(maxsize=None)
def want(name, rows_name):
    kc, nodes, pods = case(name)
    slots, word = ref.offer_slots(kc, nodes, pods, ref.row_lists(abi.table_len(pods))[rows_name])
    slots.setflags(write=False)
    word.setflags(write=False)
    return slots, word


@functools.lru_cache(maxsize=None)
def small_sets():
    kc, nodes, pods = case("small")
    ver = oracle_lib.eval_verify(kc, nodes, pods)
    mask, pod_set, bits, kind = sets_ref.kind_masks(ver.status, ver.total)
    for a in (mask, pod_set, bits, kind):
        a.setflags(write=False)
    return ver, mask, pod_set, bits, kind


def make(ctx, name, index_base=0):
    kc, nodes, pods = case(name)
    return engine.Snapshot(ctx, kc, nodes, index_base), engine.PodBatch(ctx, pods)


def check(got, exp, what):
    slots, word = got
    assert slots.dtype == np.uint32 and word.dtype == np.uint32 and slots.shape == exp[0].shape == word.shape
    assert np.array_equal(slots, exp[0]), (what, "slots", np.flatnonzero(slots != exp[0])[:6])
    assert np.array_equal(word, exp[1]), (what, "status", np.flatnonzero(word != exp[1])[:6])


# ---- 1. parity ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ref.CLUSTERS))
def test_parity(ctx, name):
    kc, nodes, pods = case(name)
    lists = ref.row_lists(abi.table_len(pods))
    if name in DISCRIMINATING:  # from the reference alone: the inputs tell the loop from its wrong readings
        slots = want(name, "head")[0]
        no_acc = int((slots != ref.plain_slots(kc, nodes, pods, lists["head"])).sum())
        full = int((slots != ref.assume_slots(kc, nodes, pods, lists["head"])).sum())
        print(f"{name}: {no_acc} nodes differ from no accumulation, {full} from the full Assume")
        assert no_acc >= 5 and full >= 5, (no_acc, full)
    snap, pb = make(ctx, name)
    for rows_name, rows in lists.items():
        exp = want(name, rows_name)
        n_rows = pb.n if rows is None else len(rows)
        assert exp[0].max() <= n_rows and ((exp[1] == 0) == (exp[0] == n_rows)).all()
        check(engine.eval_offer_slots(snap, pb, rows, status=True), exp, (name, rows_name))
        assert np.array_equal(engine.eval_offer_slots(snap, pb, rows), exp[0]), "without the status output"
    if name == "small":  # the histogram the counts are spread over
        s = want(name, "head")[0]
        assert (s == 0).sum() == 166 and (s >= 10).sum() == 124 and (s == 48).sum() == 8
        assert len(np.unique(want(name, "copies")[0])) >= 30


# ---- 2. candidate node sets --------------------------------------------------------------------------------------
def test_with_node_sets(ctx):
    kc, nodes, pods = case("small")
    ver, mask, pod_set, bits, kind = small_sets()
    snap, pb = make(ctx, "small")
    head = ref.row_lists(pb.n)["head"]
    only = np.flatnonzero(np.isin(kind, (0, 5, 6))).astype(np.uint32)  # no set, the shared half, the explicit all-true set
    plain = {"head": want("small", "head"), "only": ref.offer_slots(kc, nodes, pods, only)}
    pb.set_node_sets(pod_set, bits, snap.n)
    exp = ref.offer_slots(kc, nodes, pods, head, mask)
    assert ((exp[1] & EXCL) != 0).sum() == 134, "nodes that stop on an excluded pair"
    check(engine.eval_offer_slots(snap, pb, head, status=True), exp, "all kinds")
    exp = ref.offer_slots(kc, nodes, pods, only, mask)
    assert (exp[0] != plain["only"][0]).sum() == 65 and exp[0].max() >= 10
    check(engine.eval_offer_slots(snap, pb, only, status=True), exp, "kinds 0 / 5 / 6")
    pb.clear_node_sets()
    check(engine.eval_offer_slots(snap, pb, head, status=True), plain["head"], "sets cleared")
    check(engine.eval_offer_slots(snap, pb, only, status=True), plain["only"], "sets cleared")


# ---- 3. nothing changes ------------------------------------------------------------------------------------------
def test_nothing_changes(ctx):
    kc, nodes, pods = case("small")
    ver, mask, pod_set, bits, kind = small_sets()
    snap, pb = make(ctx, "small")
    keys = engine.eval_select(snap, pb, 3)
    status = engine.result_status(pb)
    gen = snap.generation()
    state = snap.read_state()
    check(engine.eval_offer_slots(snap, pb, status=True), want("small", "all"), "all")
    engine.eval_offer_slots(snap, pb, [3, 3, 0])
    assert np.array_equal(engine.result_keys(pb, 3), keys)
    assert np.array_equal(engine.result_status(pb), status)
    assert snap.generation() == gen
    after = snap.read_state()
    assert state.keys() == after.keys()
    for k in state:
        assert np.array_equal(state[k], after[k]), k
    assert np.array_equal(engine.eval_select(snap, pb, 3), oracle_lib.select(kc, nodes, pods, 3))
    # host score terms are ignored: Filter only
    terms = node_scores_ref.kind_terms(ver.status, ver.total)[:4]
    pb.set_node_scores(*terms, snap.n)
    check(engine.eval_offer_slots(snap, pb, status=True), want("small", "all"), "with host score terms")
    check(engine.eval_offer_slots(snap, pb, ref.row_lists(pb.n)["copies"], status=True), want("small", "copies"),
          "copies, with host score terms")


# ---- 4. layout and shards ----------------------------------------------------------------------------------------
def test_after_rows_moved_between_storage_classes(ctx):
    kc, nodes, pods = case("small")
    snap, pb = make(ctx, "small")
    head = ref.row_lists(pb.n)["head"]
    check(engine.eval_offer_slots(snap, pb, head, status=True), want("small", "head"), "before")
    single = np.flatnonzero(nodes["numa_policy"] == abi.KG_NUMA_SINGLE_NODE)
    other = np.flatnonzero(nodes["numa_policy"] != abi.KG_NUMA_SINGLE_NODE)
    rows = np.array(sorted({int(single[0]), int(other[0]), int(other[-1])}), np.uint32)
    upd = abi.take(nodes, rows.astype(np.int64))
    upd["numa_policy"] = np.where(upd["numa_policy"] == abi.KG_NUMA_SINGLE_NODE, abi.KG_NUMA_NONE,
                                  abi.KG_NUMA_SINGLE_NODE).astype(np.uint32)
    upd["num_pods"] = upd["alloc_pods"].copy()  # and are full: their counts drop to 0 with "Too many pods"
    snap.update_rows(rows, upd)  # three nodes move to the other storage class: every record between them shifts
    merged = {k: (v if k in abi.TABLE_KEYS else v.copy()) for k, v in nodes.items()}
    for k in upd:
        if k not in abi.TABLE_KEYS:
            merged[k][rows] = upd[k]
    exp = ref.offer_slots(kc, merged, pods, head)
    assert not np.array_equal(exp[0], want("small", "head")[0]) or not np.array_equal(exp[1], want("small", "head")[1])
    check(engine.eval_offer_slots(snap, pb, head, status=True), exp, "after the update")


def test_shards_concatenate_and_index_base_is_not_added(ctx):
    kc, nodes, pods = case("small")
    n = abi.table_len(nodes)
    pb = engine.PodBatch(ctx, pods)
    head = ref.row_lists(pb.n)["head"]
    halves = [np.arange(0, 150), np.arange(150, n)]
    got = [engine.eval_offer_slots(engine.Snapshot(ctx, kc, abi.take(nodes, idx), int(idx[0])), pb, head, status=True)
           for idx in halves]
    check((np.concatenate([g[0] for g in got]), np.concatenate([g[1] for g in got])), want("small", "head"), "halves")
    snap = engine.Snapshot(ctx, kc, nodes, 1000)
    check(engine.eval_offer_slots(snap, pb, head, status=True), want("small", "head"), "index_base 1000")


# ---- 5. arguments and refusals -----------------------------------------------------------------------------------
def test_arguments(ctx):
    kc, nodes, pods = case("n129")
    snap, pb = make(ctx, "n129")
    L, P = ctx.L, C.POINTER(C.c_uint32)
    slots = np.zeros(snap.n, np.uint32)
    word = np.zeros(snap.n, np.uint32)
    row0 = np.zeros(1, np.uint32)
    sp, wp, rp = slots.ctypes.data_as(P), word.ctypes.data_as(P), row0.ctypes.data_as(P)
    bad = [
        lambda: ctx.check(L.kg_eval_offer_slots(snap.h, pb.h, None, pb.n, None, wp), "null slots"),
        lambda: ctx.check(L.kg_eval_offer_slots(snap.h, pb.h, rp, 0, None, None), "null slots, no rows"),
        lambda: engine.eval_offer_slots(snap, pb, [pb.n]),
        lambda: engine.eval_offer_slots(snap, pb, [0, 0xFFFFFFFF]),
        lambda: ctx.check(L.kg_eval_offer_slots(snap.h, pb.h, None, pb.n - 1, sp, wp), "n_rows"),
        lambda: ctx.check(L.kg_eval_offer_slots(snap.h, pb.h, None, 0, sp, wp), "n_rows 0, no rows"),
    ]
    for call in bad:
        with pytest.raises(engine.EngineError) as ei:
            call()
        assert ei.value.status == abi.KG_INVALID_ARG
        assert "koordgpu" in str(ei.value)
    # n_rows == 0: zeros to both outputs, and to the slots alone
    guard = np.full(2 * snap.n + 2, 0xDEADBEEF, np.uint32)
    ctx.check(L.kg_eval_offer_slots(snap.h, pb.h, rp, 0, guard.ctypes.data_as(P), guard[snap.n + 1:].ctypes.data_as(P)),
              "n_rows 0")
    assert not guard[:snap.n].any() and not guard[snap.n + 1:2 * snap.n + 1].any()
    assert guard[snap.n] == 0xDEADBEEF and guard[-1] == 0xDEADBEEF
    got = engine.eval_offer_slots(snap, pb, [], status=True)
    assert got[0].shape == (snap.n,) and not got[0].any() and not got[1].any()
    # guard words behind the outputs of a full call stay intact
    guard[:] = 0xDEADBEEF
    ctx.check(L.kg_eval_offer_slots(snap.h, pb.h, None, pb.n, guard.ctypes.data_as(P),
                                    guard[snap.n + 1:].ctypes.data_as(P)), "guarded")
    exp = want("n129", "all")
    check((guard[:snap.n], guard[snap.n + 1:2 * snap.n + 1]), exp, "guarded")
    assert guard[snap.n] == 0xDEADBEEF and guard[-1] == 0xDEADBEEF
    guard[:] = 0xDEADBEEF
    ctx.check(L.kg_eval_offer_slots(snap.h, pb.h, None, pb.n, guard.ctypes.data_as(P), None), "no status output")
    assert np.array_equal(guard[:snap.n], exp[0]) and (guard[snap.n:] == 0xDEADBEEF).all()
    # node sets over another node count: found by the evaluating call
    ver = oracle_lib.eval_verify(kc, nodes, pods)
    mask, pod_set, bits, kind = sets_ref.kind_masks(ver.status, ver.total)
    from koordinator_amd import nodesets
    pb.set_node_sets(pod_set, nodesets.pack(np.zeros((len(bits), snap.n + 1), bool)), snap.n + 1)
    with pytest.raises(engine.EngineError) as e:
        engine.eval_offer_slots(snap, pb)
    assert e.value.status == abi.KG_INVALID_ARG
    pb.clear_node_sets()
    check(engine.eval_offer_slots(snap, pb, status=True), exp, "the context still works")


def test_snapshot_of_no_nodes(ctx):
    kc, nodes, pods = case("n33")
    snap0 = engine.Snapshot(ctx, kc, abi.take(nodes, np.zeros(0, np.int64)))
    pb = engine.PodBatch(ctx, pods)
    L, P = ctx.L, C.POINTER(C.c_uint32)
    guard = np.full(4, 0xDEADBEEF, np.uint32)
    ctx.check(L.kg_eval_offer_slots(snap0.h, pb.h, None, pb.n, guard.ctypes.data_as(P), guard[2:].ctypes.data_as(P)),
              "0 nodes")
    ctx.check(L.kg_eval_offer_slots(snap0.h, pb.h, None, pb.n, None, None), "0 nodes, null outputs")
    assert (guard == 0xDEADBEEF).all()
    got = engine.eval_offer_slots(snap0, pb, status=True)
    assert got[0].shape == (0,) and got[1].shape == (0,)


def test_config5_snapshot_is_unsupported(ctx):
    cfg, nodes, pods, quotas, rsv = synth.cluster5(64, 16, seed_config=12)
    kc = cfg.kg_config()
    snap5 = engine.Snapshot(ctx, kc, nodes)
    snap5.upload_quotas(quotas)
    if kc.plugins & abi.KG_PLUGIN_RSV:
        snap5.upload_reservations(rsv)
    pb5 = engine.PodBatch(ctx, pods)
    with pytest.raises(engine.Unsupported) as e:
        engine.eval_offer_slots(snap5, pb5)
    assert e.value.status == abi.KG_UNSUPPORTED and "config-5" in str(e.value)
    snap, pb = make(ctx, "n33")
    check(engine.eval_offer_slots(snap, pb, status=True), want("n33", "all"), "a plain call afterwards")


# ---- 6. the planner, end to end ----------------------------------------------------------------------------------
def topology_of(names):
    """nodes -> blocks of 8 -> spines of 4 blocks -> the cluster."""
    root = batch.TopologyNode("ClusterLayer", "cluster")
    for i, name in enumerate(names):
        s, b = f"spine-{i // 32:02d}", f"block-{i // 8:03d}"
        spine = root.children.get(s) or root.add_child(batch.TopologyNode("SpineLayer", s))
        block = spine.children.get(b) or spine.add_child(batch.TopologyNode("BlockLayer", b))
        block.add_child(batch.TopologyNode(batch.NODE_TOPOLOGY_LAYER, name))
    return root


def test_topology_planner_end_to_end(ctx):
    kc, nodes, pods = case("small")
    names = [f"node-{i:04d}" for i in range(abi.table_len(nodes))]
    root = topology_of(names)
    snap = engine.Snapshot(ctx, kc, nodes)
    # A gang of 40 copies of pod 36: its plan spans four nodes of one block. The reference's loop leaves the LoadAware
    # bases alone, so not every plan survives the batch cycle's whole Reserve (40 copies of pod 3 do not); this one
    # does on the oracle, which is asserted below before the device is asked
    job = abi.take(pods, np.full(40, 36, np.int64))
    members = [batch.JobPod("team", f"worker-{j:02d}", uid=f"u{j}") for j in range(40)]
    req = batch.JobTopologyRequirements("SpineLayer", 40)
    planner, sched = batch.TopologyPlanner(snap, names, root), batch.BatchScheduler(snap, names)
    plan, status, slots = planner.find_one_node(members, job, req)
    ref_slots, ref_word = ref.offer_slots(kc, nodes, job)
    assert np.array_equal(slots, ref_slots)
    exp, msg = batch.place_pods(root, dict(zip(names, map(int, ref_slots))), req, members)
    assert exp is not None and msg == ""
    assert status.is_success() and plan.pod_to_node_name == exp and [p.key for p in plan.pods] == [m.key for m in members]
    used = sorted(set(exp.values()))
    assert len({n // 32 for n in map(names.index, used)}) == 1, "gathered under one spine"
    assert len(used) == 4
    for node in used:
        assert list(exp.values()).count(node) <= ref_slots[names.index(node)]
    by_node = [(exp[m.key], j) for j, m in enumerate(members)]  # the batch cycle's order: per node, pods by name
    cycle = [j for node in dict.fromkeys(n for n, _ in by_node) for n, j in by_node if n == node]
    res = oracle_lib.OracleState(kc, nodes).batch_schedule(
        abi.take(job, np.asarray(cycle, np.int64)), np.asarray([names.index(exp[members[j].key]) for j in cycle], np.int32))[0]
    assert (res == abi.KG_BATCH_ASSUMED).all(), "the oracle's batch cycle assumes the plan"
    # a job no block holds: the solver's message, with the FitError of the nodes' first failing plugin
    big = batch.JobTopologyRequirements("BlockLayer", 400)
    job2 = abi.take(pods, np.full(400, 3, np.int64))
    m2 = [batch.JobPod("team", f"w-{j:03d}") for j in range(400)]
    plan2, st2, slots2 = planner.find_one_node(m2, job2, big)
    assert plan2 is None and st2.code == batch.UNSCHEDULABLE
    words2 = ref.offer_slots(kc, nodes, job2)
    want_msg = batch.place_pods(root, dict(zip(names, map(int, words2[0]))), big, m2,
                                node_status={n: int(w) for n, w in zip(names, words2[1]) if w},
                                num_all_nodes=len(names))[1]
    assert st2.message == want_msg and st2.message.startswith(
        "no candidate topology nodes can accommodate job, desiredOfferSlot: 400, topology topologyNode BlockLayer/block-000: ")
    assert f"0/{len(names)} nodes are available: " in st2.message
    # the batch cycle takes the plan unchanged and assumes every pod of it
    out = sched.batch_schedule(plan, {m.key: (job, j) for j, m in enumerate(members)})
    assert out.status.is_success(), out.status.message
    assert sorted(out.assumed) == sorted(m.key for m in members)
    assert {k: v[0] for k, v in out.assumed.items()} == exp
