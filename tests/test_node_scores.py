"""Per-pod host score terms on the device (kg_pods_set_node_scores): select and verify add the host plugins' weighted
values to koord's total, against reference values built from the CPU oracle's verify matrix (node_scores_ref).

Bar: bit-exact (np.array_equal): keys, totals and status words are integers.

Term kinds, dealt by j % 8 (node_scores_ref.kind_terms): 0 none, 1 RAW on the second-best node, 2 NORMALIZE with its
largest raw on an infeasible node, 3 NORMALIZE_REVERSE with maximum 0, 4 NORMALIZE_REVERSE with its largest raw on an
infeasible node, 5 all four slots, 6 a shared NORMALIZE row plus a per-pod RAW row, 7 a tie. Kinds 1, 2, 4 and 5 move
every pod to its second-best node; kind 0 must equal the oracle's select row for row."""
import functools

import numpy as np
import pytest

import node_scores_ref as ref
import node_sets_ref as sets_ref
import oracle_lib
from koordinator_amd import abi, engine, nodescores, nodesets, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def case(name):
    """(kg_config, nodes, pods, the oracle's verify result, terms (pod_terms, raw, mode, weight), kind, second) of one
    cluster; read-only."""
    cfg, nodes, pods = ref.CLUSTERS[name](synth)
    kc = cfg.kg_config()
    ver = oracle_lib.eval_verify(kc, nodes, pods)
    pod_terms, raw, mode, weight, kind, first, second = ref.kind_terms(ver.status, ver.total)
    for a in (ver.status, ver.total, pod_terms, raw, mode, weight):
        a.setflags(write=False)
    return kc, nodes, pods, ver, (pod_terms, raw, mode, weight), kind, second


@functools.lru_cache(maxsize=None)
def want_keys(name, k):
    kc, nodes, pods, ver, terms, kind, second = case(name)
    return ref.expected_keys(ver.status, ver.total, None, k, *terms)


def with_terms(ctx, name):
    kc, nodes, pods, ver, terms, kind, second = case(name)
    snap = engine.Snapshot(ctx, kc, nodes)
    batch = engine.PodBatch(ctx, pods)
    batch.set_node_scores(*terms, snap.n)
    return snap, batch


# ---- select ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("name", list(ref.CLUSTERS))
def test_select_keys(ctx, name, k):
    kc, nodes, pods, ver, terms, kind, second = case(name)
    snap, batch = with_terms(ctx, name)
    got = engine.eval_select(snap, batch, k)
    want = want_keys(name, k)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    plain = oracle_lib.select(kc, nodes, pods, k)
    assert np.array_equal(got[kind == 0], plain[kind == 0])
    moved = np.isin(kind, (1, 2, 4, 5))
    assert (abi.key_node(got[moved, 0]) != abi.key_node(plain[moved, 0])).all() and moved.sum() >= 4
    assert np.array_equal(abi.key_node(got[moved, 0]), second[moved])
    flagged = engine.result_status(batch)
    unsup = ((ver.status & abi.KG_ST_UNSUPPORTED) != 0).any(axis=1)
    assert not flagged[~unsup].any()
    assert not (flagged & ~np.uint32(abi.KG_ST_UNSUPPORTED)).any()


@pytest.mark.parametrize("name", list(ref.CLUSTERS))
def test_terms_with_sets(ctx, name):
    kc, nodes, pods, ver, terms, kind, second = case(name)
    mask, pod_set, bits, set_kind = sets_ref.kind_masks(ver.status, ver.total)  # j % 7 against the terms' j % 8
    snap, batch = with_terms(ctx, name)
    batch.set_node_sets(pod_set, bits, snap.n)
    for k in (1, 3):
        got = engine.eval_select(snap, batch, k)
        want = ref.expected_keys(ver.status, ver.total, mask, k, *terms)
        assert np.array_equal(got, want), (k, np.argwhere(got != want)[:4])
    assert not got[(set_kind == 2) | (set_kind == 3)].any(), "no feasible candidate: keys 0"
    assert (got[(set_kind == 0) | (set_kind == 6)] == want_keys(name, 3)[(set_kind == 0) | (set_kind == 6)]).all()


def test_maximum_on_a_feasible_node_the_set_excludes(ctx):
    kc, nodes, pods, ver, *_ = case("small")
    p, n = ver.status.shape
    top3 = sets_ref.expected_keys(ver.status, ver.total, None, 3)
    first, second, third = (abi.key_node(top3[:, t]) for t in range(3))
    assert (third >= 0).all()
    mask = np.ones((p, n), bool)
    lists = []
    for j in range(p):  # NORMALIZE w2: 1000 on the best node, which the set excludes, 10 on the third-best
        raw = np.zeros(n, np.int32)
        raw[first[j]], raw[third[j]] = 1000, 10
        lists.append([(raw, ref.NORM, 2)])
        mask[j, first[j]] = False
    terms = nodescores.from_terms(lists, n)
    snap = engine.Snapshot(ctx, kc, nodes)
    batch = engine.PodBatch(ctx, pods)
    batch.set_node_scores(*terms, n)
    batch.set_node_sets(*nodesets.from_mask(mask), n)
    got = engine.eval_select(snap, batch, 1)
    assert np.array_equal(got, ref.expected_keys(ver.status, ver.total, mask, 1, *terms))
    assert np.array_equal(abi.key_node(got[:, 0]), third), "the maximum over the candidates is 10: +200 on the third-best"
    # an empty set: keys 0
    batch.set_node_sets(np.zeros(p, np.int32), nodesets.pack(np.zeros((1, n), bool)), n)
    assert not engine.eval_select(snap, batch, 3).any()


@pytest.mark.parametrize("shared", [True, False])
def test_uniform_and_mixed_waves(ctx, shared):
    kc, nodes, pods, ver, *_ = case("small")
    p, n = ver.status.shape
    rng = np.random.default_rng(17)
    one = rng.integers(0, 1001, n).astype(np.int32)
    lists = [[(one if shared else rng.integers(0, 1001, n).astype(np.int32), ref.NORM, 1),
              (one if shared else rng.integers(0, 40, n).astype(np.int32), ref.RAW, 2)] for _ in range(p)]
    terms = nodescores.from_terms(lists, n)
    assert len(terms[1]) == (2 if shared else 2 * p)
    snap = engine.Snapshot(ctx, kc, nodes)
    batch = engine.PodBatch(ctx, pods)
    batch.set_node_scores(*terms, n)
    for k in (1, 3):
        assert np.array_equal(engine.eval_select(snap, batch, k), ref.expected_keys(ver.status, ver.total, None, k, *terms)), k


@pytest.mark.parametrize("name", ["small", "mixed"])
def test_integer_path_gives_the_same_keys(ctx, name, monkeypatch):
    snap, batch = with_terms(ctx, name)
    monkeypatch.setenv("KG_SELECT_INT", "1")  # read per call
    for k in (1, 3):
        assert np.array_equal(engine.eval_select(snap, batch, k), want_keys(name, k)), k


# ---- verify, diagnose, feasible ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "mixed"])
def test_verify(ctx, name):
    kc, nodes, pods, ver, terms, kind, second = case(name)
    snap, batch = with_terms(ctx, name)
    got = engine.eval_verify(snap, batch)
    want = ref.expected_verify_total(ver.status, ver.total, None, *terms)
    assert np.array_equal(got.total, want)
    assert (got.total[ver.status != 0] == -1).all() and (want != ver.total).sum() > 1000
    for col in ("status", "score_nrf", "score_la", "score_numa", "numa_zone"):
        assert np.array_equal(getattr(got, col), getattr(ver, col)), col
    # with sets: the maxima follow the candidates, an excluded pair's total is -1
    mask, pod_set, bits, _ = sets_ref.kind_masks(ver.status, ver.total)
    batch.set_node_sets(pod_set, bits, snap.n)
    got = engine.eval_verify(snap, batch)
    assert np.array_equal(got.total, ref.expected_verify_total(ver.status, ver.total, mask, *terms))
    assert np.array_equal(got.status, sets_ref.expected_status(ver.status, mask))


def test_diagnose_and_feasible_ignore_the_terms(ctx):
    kc, nodes, pods, ver, terms, kind, second = case("small")
    snap, batch = with_terms(ctx, "small")
    plain = engine.PodBatch(ctx, pods)
    for first_plugin in (False, True):
        assert np.array_equal(engine.eval_diagnose(snap, batch, first_plugin=first_plugin),
                              engine.eval_diagnose(snap, plain, first_plugin=first_plugin))
    bits = engine.eval_feasible(snap, batch)
    assert np.array_equal(bits, engine.eval_feasible(snap, plain))
    assert np.array_equal(nodesets.to_mask(bits, snap.n), ver.status == 0)


# ---- lanes -------------------------------------------------------------------------------------------------------
def test_dedup_counts_the_term_tuple_into_the_row(ctx):
    kc, nodes, pods, ver, *_ = case("small")
    n = abi.table_len(nodes)
    # 4 distinct rows of fast lanes (no NUMA policy of their own, no cpuset bind) x 32 copies
    fast = np.flatnonzero((pods["numa_policy"] == 0) & ((pods["flags"] & abi.KG_POD_CPU_BIND) == 0))
    _, first = np.unique(np.stack([pods["req_cpu"][fast], pods["req_mem"][fast]]), axis=1, return_index=True)
    four = fast[np.sort(first)[:4]]
    assert len(four) == 4
    tiled = np.tile(four, 32)
    rows = abi.take(pods, tiled)
    rng = np.random.default_rng(23)
    a, b, c = (rng.integers(0, 1001, n).astype(np.int32) for _ in range(3))
    tuples = ([(a, ref.NORM, 1), (b, ref.RAW, 1)], [(c, ref.REV, 2)])
    # the tuples alternate every four pods, so that every row meets both: 4 rows x 2 tuples
    terms = nodescores.from_terms([tuples[j // 4 % 2] for j in range(128)], n)
    assert len(terms[1]) == 3
    snap = engine.Snapshot(ctx, kc, nodes)
    batch = engine.PodBatch(ctx, rows)
    assert batch.select_lanes()[0] == 4
    batch.set_node_scores(*terms, n)
    assert batch.select_lanes()[0] == 8
    st, tot = ver.status[tiled], ver.total[tiled]
    for k in (1, 3):
        assert np.array_equal(engine.eval_select(snap, batch, k), ref.expected_keys(st, tot, None, k, *terms)), k
    batch.clear_node_scores()
    assert batch.select_lanes()[0] == 4
    for k in (1, 3):
        assert np.array_equal(engine.eval_select(snap, batch, k), sets_ref.expected_keys(st, tot, None, k)), k


def test_layout_change_rebuilds_the_table(ctx):
    kc, nodes, pods, ver, terms, kind, second = case("small")
    snap, batch = with_terms(ctx, "small")
    assert np.array_equal(engine.eval_select(snap, batch, 1), want_keys("small", 1))
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
        got = engine.eval_select(snap, batch, k)  # the terms are not touched
        assert np.array_equal(got, ref.expected_keys(ver2.status, ver2.total, None, k, *terms)), k


# ---- lifetime and arguments --------------------------------------------------------------------------------------
def test_lifetime(ctx):
    kc, nodes, pods, ver, terms, kind, second = case("n129")
    mask, pod_set, bits, _ = sets_ref.kind_masks(ver.status, ver.total)
    plain = oracle_lib.select(kc, nodes, pods, 1)
    snap, batch = with_terms(ctx, "n129")
    assert np.array_equal(engine.eval_select(snap, batch, 1), want_keys("n129", 1))
    batch.upload(pods)  # an upload clears the terms
    assert np.array_equal(engine.eval_select(snap, batch, 1), plain)
    batch.set_node_scores(*terms, snap.n)
    batch.clear_node_scores()  # and so does NULL
    assert np.array_equal(engine.eval_select(snap, batch, 1), plain)
    # clearing the terms keeps the sets, and the other way round
    batch.set_node_scores(*terms, snap.n)
    batch.set_node_sets(pod_set, bits, snap.n)
    batch.clear_node_scores()
    assert np.array_equal(engine.eval_select(snap, batch, 1), sets_ref.expected_keys(ver.status, ver.total, mask, 1))
    batch.set_node_scores(*terms, snap.n)
    batch.clear_node_sets()
    assert np.array_equal(engine.eval_select(snap, batch, 1), want_keys("n129", 1))
    batch.clear_node_scores()
    assert np.array_equal(engine.eval_select(snap, batch, 1), plain)
    assert not engine.result_status(batch).any()


def test_argument_checks(ctx):
    kc, nodes, pods, ver, (pod_terms, raw, mode, weight), kind, second = case("n129")
    snap = engine.Snapshot(ctx, kc, nodes)
    n, rows = snap.n, len(raw)

    def refused(*terms):
        with pytest.raises(engine.EngineError) as e:
            batch.set_node_scores(*terms)
        assert e.value.status == abi.KG_INVALID_ARG
        assert np.array_equal(engine.eval_select(snap, batch, 1), want_keys("n129", 1)), "the terms in force stay"

    import ctypes as C
    h = C.c_void_p()  # a batch that was never uploaded
    ctx.check(ctx.L.kg_pods_create(ctx.h, 4, C.byref(h)), "kg_pods_create")
    i32p, u32p = C.POINTER(C.c_int32), C.POINTER(C.c_uint32)
    sc = abi.KgNodeScores(np.full(4, -1, np.int32).ctypes.data_as(i32p), raw.ctypes.data_as(i32p),
                          mode.ctypes.data_as(u32p), weight.ctypes.data_as(u32p), rows, n)
    assert ctx.L.kg_pods_set_node_scores(h, C.byref(sc)) == abi.KG_INVALID_ARG
    assert ctx.L.kg_pods_set_node_scores(h, None) == abi.KG_INVALID_ARG
    ctx.L.kg_pods_destroy(h)

    batch = engine.PodBatch(ctx, pods)
    batch.set_node_scores(pod_terms, raw, mode, weight, n)
    hi, lo = pod_terms.copy(), pod_terms.copy()
    hi[1, 0], lo[1, 0] = rows, -2
    refused(hi, raw, mode, weight, n)
    refused(lo, raw, mode, weight, n)
    neg, big = raw.copy(), raw.copy()
    neg[0, 5], big[0, 5] = -1, abi.KG_SCORE_RAW_MAX + 1
    refused(pod_terms, neg, mode, weight, n)
    refused(pod_terms, big, mode, weight, n)
    m3, w = mode.copy(), weight.copy()
    m3[0], w[0] = 3, (1 << 20) + 1
    refused(pod_terms, raw, m3, weight, n)
    refused(pod_terms, raw, mode, w, n)
    at_max = raw.copy()
    at_max[0, 5] = abi.KG_SCORE_RAW_MAX  # the bounds themselves are accepted
    w[0] = 0
    batch.set_node_scores(pod_terms, at_max, mode, w, n)
    batch.set_node_scores(pod_terms, raw, mode, weight, n)

    def evaluating_calls_refuse():
        for call in (lambda: engine.eval_select(snap, batch, 1), lambda: engine.eval_verify(snap, batch)):
            with pytest.raises(engine.EngineError) as e:
                call()
            assert e.value.status == abi.KG_INVALID_ARG

    # rows over another node count are found by the evaluating call
    batch.set_node_scores(pod_terms, np.zeros((rows, n + 1), np.int32), mode, weight, n + 1)
    evaluating_calls_refuse()
    # the total field of the packed key: the snapshot's sum of weights x 100 plus the largest per-pod bound
    wsum = 100 * (kc.weight_nrf + kc.weight_la + kc.weight_numa + kc.weight_dev + kc.weight_rsv)
    one = np.full((len(pods["req_cpu"]), 4), -1, np.int32)
    one[:, 0] = 0
    flat = np.full((1, n), 1 << 12, np.int32)
    fits = ((1 << 31) - 1 - wsum) >> 12
    assert fits <= 1 << 20
    batch.set_node_scores(one, flat, [abi.KG_SCORE_RAW], [fits + 1], n)
    evaluating_calls_refuse()
    batch.set_node_scores(one, flat, [abi.KG_SCORE_RAW], [fits], n)
    got = engine.eval_select(snap, batch, 1)  # a constant on every node: the oracle's nodes, larger totals
    plain = oracle_lib.select(kc, nodes, pods, 1)
    assert np.array_equal(abi.key_node(got), abi.key_node(plain))
    assert np.array_equal(abi.key_total(got), abi.key_total(plain) + (fits << 12))
    batch.set_node_scores(pod_terms, raw, mode, weight, n)
    assert np.array_equal(engine.eval_select(snap, batch, 1), want_keys("n129", 1))


# ---- refusals ----------------------------------------------------------------------------------------------------
def test_config5_snapshot_is_refused(ctx):
    cfg, nodes, pods, quotas, rsv = synth.cluster5(64, 16, seed_config=12)
    kc = cfg.kg_config()
    snap = engine.Snapshot(ctx, kc, nodes)
    snap.upload_quotas(quotas)
    if kc.plugins & abi.KG_PLUGIN_RSV:
        snap.upload_reservations(rsv)
    batch = engine.PodBatch(ctx, pods)
    want = engine.eval_select(snap, batch, 1)
    terms = nodescores.from_terms([[(np.arange(64), ref.NORM, 1)]] * 16, 64)
    batch.set_node_scores(*terms, 64)
    for call in (lambda: engine.eval_select(snap, batch, 1), lambda: engine.eval_verify(snap, batch)):
        with pytest.raises(engine.Unsupported):
            call()
    batch.clear_node_scores()
    assert np.array_equal(engine.eval_select(snap, batch, 1), want)
    engine.eval_verify(snap, batch)


def test_shard_select_is_refused():
    kc, nodes, pods, ver, terms, kind, second = case("n33")
    sctx = engine.Context(0)
    try:
        sctx.shard_init(engine.shard_unique_id(), 0, 1)
        snap = engine.Snapshot(sctx, kc, nodes)
        batch = engine.PodBatch(sctx, pods)
        batch.set_node_scores(*terms, snap.n)
        with pytest.raises(engine.Unsupported):
            engine.shard_select(snap, batch, 1)
        batch.clear_node_scores()
        assert np.array_equal(engine.shard_select(snap, batch, 1), oracle_lib.select(kc, nodes, pods, 1))
    finally:
        sctx.close()


def test_replay_is_refused(ctx):
    cfg, nodes, pods = synth.small(120, 40, scale=4.0)
    kc = cfg.kg_config()
    snap = engine.Snapshot(ctx, kc, nodes)
    batch = engine.PodBatch(ctx, pods)
    batch.set_node_scores(*nodescores.from_terms([[(np.arange(120), ref.RAW, 1)]] * 40, 120), 120)
    with pytest.raises(engine.Unsupported):
        engine.replay(snap, batch)
    batch.clear_node_scores()
    wn, wt = oracle_lib.OracleState(kc, nodes).replay(pods)[:2]
    out = engine.replay(snap, batch)
    assert np.array_equal(out[0], wn) and np.array_equal(out[1], wt)
