"""Per-pod candidate node sets on the device (kg_pods_set_node_sets): select, verify, diagnose and replay honour the
nodes the host allows each pod, against reference values built from the CPU oracle's verify matrix (node_sets_ref).

Bar: bit-exact (np.array_equal): keys, status words, counts and placements are integers.

Set kinds, dealt by j % 7 (node_sets_ref.kind_masks): 0 no set, 1 every node but the pod's unmasked winner, 2 only
nodes infeasible for the pod, 3 the empty set, 4 exactly the pod's second-best node, 5 one random half shared by all
pods of the kind, 6 an explicit all-true set. Kinds 1-4 change every pod's answer; kinds 0 and 6 must equal the
oracle's select row for row."""
import functools

import numpy as np
import pytest

import node_sets_ref as ref
import oracle_lib
from koordinator_amd import abi, engine, nodesets, synth

pytestmark = pytest.mark.gpu

EXCL = abi.KG_ST_NODE_EXCLUDED
SLOTS, DEV0, FEASIBLE = 64, 32, 48


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def case(name):
    """(kg_config, nodes, pods, the oracle's verify result, mask, pod_set, bits, kind) of one cluster; read-only."""
    cfg, nodes, pods = ref.CLUSTERS[name](synth)
    kc = cfg.kg_config()
    ver = oracle_lib.eval_verify(kc, nodes, pods)
    mask, pod_set, bits, kind = ref.kind_masks(ver.status, ver.total)
    for a in (ver.status, ver.total, mask, pod_set, bits):
        a.setflags(write=False)
    return kc, nodes, pods, ver, mask, pod_set, bits, kind


def with_sets(ctx, name):
    kc, nodes, pods, ver, mask, pod_set, bits, kind = case(name)
    snap = engine.Snapshot(ctx, kc, nodes)
    batch = engine.PodBatch(ctx, pods)
    batch.set_node_sets(pod_set, bits, snap.n)
    return snap, batch


# ---- select ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("name", list(ref.CLUSTERS))
def test_select_keys(ctx, name, k):
    kc, nodes, pods, ver, mask, pod_set, bits, kind = case(name)
    snap, batch = with_sets(ctx, name)
    got = engine.eval_select(snap, batch, k)
    want = ref.expected_keys(ver.status, ver.total, mask, k)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    # by construction: kinds 0 and 6 are the unmasked select, kinds 1-4 change every pod's answer
    plain = oracle_lib.select(kc, nodes, pods, k)
    same = (kind == 0) | (kind == 6)
    assert np.array_equal(got[same], plain[same])
    changed = (kind >= 1) & (kind <= 4) & (plain[:, 0] != 0)
    assert (got[changed, 0] != plain[changed, 0]).all() and changed.sum() >= 4
    assert not got[(kind == 2) | (kind == 3)].any(), "no feasible candidate: keys 0"
    # a pod is flagged only for a candidate pair that needs the host path
    flagged = engine.result_status(batch)
    unsup = (((ver.status & abi.KG_ST_UNSUPPORTED) != 0) & mask).any(axis=1)
    assert not (flagged[~unsup]).any()
    assert not (flagged & ~np.uint32(abi.KG_ST_UNSUPPORTED)).any()


def test_dedup_counts_the_set_into_the_row(ctx):
    kc, nodes, pods, ver, *_ = case("small")
    n = abi.table_len(nodes)
    # 4 distinct rows of fast lanes (no NUMA policy of their own, no cpuset bind) x 32 copies
    fast = np.flatnonzero((pods["numa_policy"] == 0) & ((pods["flags"] & abi.KG_POD_CPU_BIND) == 0))
    _, first = np.unique(np.stack([pods["req_cpu"][fast], pods["req_mem"][fast]]), axis=1, return_index=True)
    four = fast[np.sort(first)[:4]]
    assert len(four) == 4
    tiled = np.tile(four, 32)
    rows = abi.take(pods, tiled)
    half = np.arange(n) < n // 2
    # the sets alternate every four pods, so that every row meets both halves: 4 rows x 2 sets
    mask = np.where((np.arange(128) // 4 % 2 == 0)[:, None], half[None, :], ~half[None, :])
    pod_set, bits = nodesets.from_mask(mask)
    assert len(bits) == 2
    snap = engine.Snapshot(ctx, kc, nodes)
    batch = engine.PodBatch(ctx, rows)
    assert batch.select_lanes()[0] == 4
    batch.set_node_sets(pod_set, bits, n)
    assert batch.select_lanes()[0] == 8
    st, tot = ver.status[tiled], ver.total[tiled]
    for k in (1, 3):
        assert np.array_equal(engine.eval_select(snap, batch, k), ref.expected_keys(st, tot, mask, k)), k
    batch.clear_node_sets()
    assert batch.select_lanes()[0] == 4
    for k in (1, 3):
        assert np.array_equal(engine.eval_select(snap, batch, k), ref.expected_keys(st, tot, None, k)), k


def test_layout_change_rebuilds_the_table(ctx):
    kc, nodes, pods, ver, mask, pod_set, bits, kind = case("small")
    snap, batch = with_sets(ctx, "small")
    assert np.array_equal(engine.eval_select(snap, batch, 1), ref.expected_keys(ver.status, ver.total, mask, 1))
    single = np.flatnonzero(nodes["numa_policy"] == abi.KG_NUMA_SINGLE_NODE)
    other = np.flatnonzero(nodes["numa_policy"] != abi.KG_NUMA_SINGLE_NODE)
    rows = np.array(sorted({int(single[0]), int(other[0]), int(other[-1])}), np.uint32)
    upd = abi.take(nodes, rows.astype(np.int64))
    upd["numa_policy"] = np.where(upd["numa_policy"] == abi.KG_NUMA_SINGLE_NODE, abi.KG_NUMA_NONE,
                                  abi.KG_NUMA_SINGLE_NODE).astype(np.uint32)
    snap.update_rows(rows, upd)  # three nodes move to the other storage class: every record between them shifts
    merged = {k: v.copy() for k, v in nodes.items()}
    for k in upd:
        merged[k][rows] = upd[k]
    ver2 = oracle_lib.eval_verify(kc, merged, pods)
    for k in (1, 3):
        got = engine.eval_select(snap, batch, k)  # the sets are not touched
        assert np.array_equal(got, ref.expected_keys(ver2.status, ver2.total, mask, k)), k


# ---- lifetime and arguments --------------------------------------------------------------------------------------
def test_upload_clears_the_sets(ctx):
    kc, nodes, pods, ver, mask, pod_set, bits, kind = case("n129")
    snap, batch = with_sets(ctx, "n129")
    assert np.array_equal(engine.eval_select(snap, batch, 1), ref.expected_keys(ver.status, ver.total, mask, 1))
    batch.upload(pods)
    assert np.array_equal(engine.eval_select(snap, batch, 1), oracle_lib.select(kc, nodes, pods, 1))


def test_argument_checks(ctx):
    kc, nodes, pods, ver, mask, pod_set, bits, kind = case("n129")
    snap = engine.Snapshot(ctx, kc, nodes)
    batch = engine.PodBatch(ctx, pods)
    with pytest.raises(engine.EngineError) as e:
        batch.set_node_sets(np.where(pod_set == 0, len(bits), pod_set), bits, snap.n)  # a set id >= n_sets
    assert e.value.status == abi.KG_INVALID_ARG
    # a bitmap over another node count is found by the evaluating call
    wrong = nodesets.pack(np.zeros((len(bits), snap.n + 1), bool))
    batch.set_node_sets(pod_set, wrong, snap.n + 1)
    for call in (lambda: engine.eval_select(snap, batch, 1), lambda: engine.eval_verify(snap, batch),
                 lambda: engine.eval_diagnose(snap, batch), lambda: engine.replay(snap, batch)):
        with pytest.raises(engine.EngineError) as e:
            call()
        assert e.value.status == abi.KG_INVALID_ARG


def test_config5_snapshot_is_refused(ctx):
    cfg, nodes, pods, quotas, rsv = synth.cluster5(64, 16, seed_config=12)
    kc = cfg.kg_config()
    snap = engine.Snapshot(ctx, kc, nodes)
    snap.upload_quotas(quotas)
    if kc.plugins & abi.KG_PLUGIN_RSV:
        snap.upload_reservations(rsv)
    batch = engine.PodBatch(ctx, pods)
    engine.eval_select(snap, batch, 1)
    mask = np.ones((16, 64), bool)
    mask[:, ::2] = False
    batch.set_node_sets(*nodesets.from_mask(mask), 64)
    for call in (lambda: engine.eval_select(snap, batch, 1), lambda: engine.eval_verify(snap, batch),
                 lambda: engine.eval_diagnose(snap, batch), lambda: engine.replay(snap, batch)):
        with pytest.raises(engine.Unsupported):
            call()
    batch.clear_node_sets()
    engine.eval_select(snap, batch, 1)


def test_shard_select_is_refused():
    kc, nodes, pods, ver, mask, pod_set, bits, kind = case("n33")
    sctx = engine.Context(0)
    try:
        sctx.shard_init(engine.shard_unique_id(), 0, 1)
        snap = engine.Snapshot(sctx, kc, nodes)
        batch = engine.PodBatch(sctx, pods)
        batch.set_node_sets(pod_set, bits, snap.n)
        with pytest.raises(engine.Unsupported):
            engine.shard_select(snap, batch, 1)
        batch.clear_node_sets()
        assert np.array_equal(engine.shard_select(snap, batch, 1), oracle_lib.select(kc, nodes, pods, 1))
    finally:
        sctx.close()


# ---- the unsupported flag follows the candidates -----------------------------------------------------------------
def test_unsupported_flag_is_restricted_to_candidates(ctx):
    cfg, nodes, pods = synth.mixed(240, 160, seed=31)
    rng = np.random.default_rng(31)
    marked = dict(nodes)
    marked["rsv_numa"] = (rng.random(240) < 0.3).astype(np.uint8)  # the cluster of test_rsv_numa.py
    kc = cfg.kg_config()
    want = oracle_lib.eval_verify(kc, marked, pods)
    snap = engine.Snapshot(ctx, kc, marked)
    batch = engine.PodBatch(ctx, pods)
    engine.eval_select(snap, batch, 1)
    today = engine.result_status(batch)
    chosen = np.flatnonzero(today & abi.KG_ST_UNSUPPORTED)[:2]
    assert len(chosen) == 2
    mask = np.tile((marked["rsv_numa"] == 0)[None, :], (160, 1))  # every pod: the unmarked nodes only
    mask[chosen] = True                                             # but two flagged pods keep every node
    assert not (((want.status & abi.KG_ST_UNSUPPORTED) != 0) & mask)[np.setdiff1d(np.arange(160), chosen)].any()
    batch.set_node_sets(*nodesets.from_mask(mask), 240)
    for k in (1, 3):
        assert np.array_equal(engine.eval_select(snap, batch, k), ref.expected_keys(want.status, want.total, mask, k)), k
        status = engine.result_status(batch)
        assert np.array_equal(status[chosen], today[chosen]) and status[chosen].all()
        status[chosen] = 0
        assert not status.any()


# ---- verify ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "mixed"])
def test_verify(ctx, name):
    kc, nodes, pods, ver, mask, pod_set, bits, kind = case(name)
    snap, batch = with_sets(ctx, name)
    got = engine.eval_verify(snap, batch)
    assert np.array_equal(got.status, ref.expected_status(ver.status, mask))
    assert np.array_equal(got.total, np.where(mask, ver.total, -1))
    for col in ("score_nrf", "score_la", "score_numa", "numa_zone"):
        assert np.array_equal(getattr(got, col), getattr(ver, col)), col
    assert (~mask).sum() > 1000 and ((ver.status == 0) & ~mask).any()


# ---- diagnose ----------------------------------------------------------------------------------------------------
def counts(words):
    out = np.zeros((words.shape[0], SLOTS), np.uint32)
    for b in range(32):
        out[:, b] = ((words >> np.uint32(b)) & np.uint32(1)).sum(axis=1)
    code = ((words >> np.uint32(24)) & np.uint32(3)) | (((words >> np.uint32(6)) & np.uint32(3)) << np.uint32(2))
    for c in range(1, 16):
        out[:, DEV0 + c] = (code == c).sum(axis=1)
    out[:, FEASIBLE] = (words == 0).sum(axis=1)
    return out


def first_group(words):
    """The counted word of KG_DIAG_FIRST_PLUGIN: the quota gate, the excluded bit, then the filter order."""
    groups = (abi.KG_ST_QUOTA, EXCL, abi.KG_ST_NRF_MASK, abi.KG_ST_LA_MASK, abi.KG_ST_NUMA_MASK | abi.KG_ST_UNSUPPORTED,
              abi.KG_ST_DEV_MASK | abi.KG_ST_DEV_RSV, abi.KG_ST_RSV_MASK)
    m = words.copy()
    for g in reversed(groups):
        m = np.where((words & np.uint32(g)) != 0, np.uint32(g), m)
    return words & m


@pytest.mark.parametrize("first_plugin", [False, True])
def test_diagnose(ctx, first_plugin):
    kc, nodes, pods, ver, mask, pod_set, bits, kind = case("small")
    snap, batch = with_sets(ctx, "small")
    words = ref.expected_status(ver.status, mask)
    want = counts(first_group(words) if first_plugin else words)
    got = engine.eval_diagnose(snap, batch, first_plugin=first_plugin)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    assert np.array_equal(got[:, 15], (~mask).sum(axis=1)), "slot 15: the excluded nodes"
    assert np.array_equal(got[:, FEASIBLE], ((ver.status == 0) & mask).sum(axis=1)), "feasible candidates only"
    if first_plugin:  # an excluded node adds to no other slot
        inside = counts(first_group(np.where(mask, ver.status, np.uint32(1 << 30))))  # excluded nodes parked on an unused bit
        inside[:, 30] = 0
        other = got.copy()
        other[:, 15] = 0
        assert np.array_equal(other, inside)
    rows = np.array([9, 3, 3, 60], np.uint32)
    assert np.array_equal(engine.eval_diagnose(snap, batch, rows, first_plugin=first_plugin), want[rows])


# ---- replay ------------------------------------------------------------------------------------------------------
def test_replay(ctx):
    cfg, nodes, pods = synth.small(120, 40, scale=4.0)
    kc = cfg.kg_config()
    plain_state = oracle_lib.OracleState(kc, nodes)
    pn, pt, pr = plain_state.replay(pods, reasons=True)
    ver = oracle_lib.eval_verify(kc, nodes, pods)
    mask, pod_set, bits, kind = ref.kind_masks(ver.status, ver.total, winner=pn)
    wn, wt, wr, wstate = ref.step_replay(kc, nodes, pods, mask)
    assert (wn != pn).sum() >= 5 and (wr & EXCL).any() and not (wr[kind == 0] & EXCL).any()
    for reasons in (True, False):
        snap = engine.Snapshot(ctx, kc, nodes)
        batch = engine.PodBatch(ctx, pods)
        batch.set_node_sets(pod_set, bits, snap.n)
        out = engine.replay(snap, batch, reasons=reasons)
        assert np.array_equal(out[0], wn) and np.array_equal(out[1], wt), reasons
        if reasons:
            assert np.array_equal(out[2], wr)
        state, want = snap.read_state(), wstate.table()
        for key in ref.STATE_KEYS:
            assert np.array_equal(state[key], want[key]), key
        # the same batch without sets on the same snapshot, uploaded again (same device buffers): the cached replay
        # graph is not reused across the change
        batch.clear_node_sets()
        snap.upload(nodes)
        out = engine.replay(snap, batch, reasons=reasons)
        assert np.array_equal(out[0], pn) and np.array_equal(out[1], pt), reasons
        if reasons:
            assert np.array_equal(out[2], pr)
        state, want = snap.read_state(), plain_state.table()
        for key in ref.STATE_KEYS:
            assert np.array_equal(state[key], want[key]), key
