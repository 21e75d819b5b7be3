"""kg_eval_feasible on the device: per requested pod, one bit per node of the snapshot (the pair's status word has no
bit of fail_mask), against the CPU oracle's verify status matrix.

Bar: bit-exact (np.array_equal) on the 32-bit words, padding bits included. The expected bitmap is
nodesets.pack((oracle_status & fail_mask) == 0); with candidate node sets the oracle's word takes KG_ST_NODE_EXCLUDED
first (node_sets_ref.expected_status).

Clusters (pods x nodes, feasible share, distinct status words; from the oracle):
  small   64 x 300  0.72  11   both storage classes
  mixed  160 x 240  0.73  13   F_BIG records
  n33      8 x 33   0.79   6   a last word of one bit
  n129    70 x 129  0.77   8   class boundary off the 64-record grid, more than one wave of rows
  c5_64   16 x 64   0.59   7  config 5, two pods without a feasible node
  c5_200  70 x 200  0.66  52   config 5
No pod has every node feasible and no pair is unsupported in any of them."""
import ctypes as C
import functools

import numpy as np
import pytest

import node_sets_ref as ref
import oracle_lib
from koordinator_amd import abi, engine, nodesets, synth

pytestmark = pytest.mark.gpu

ALL = 0xFFFFFFFF
EXCL = abi.KG_ST_NODE_EXCLUDED
MASKS = [ALL, abi.KG_ST_NRF_MASK, abi.KG_ST_UNRESOLVABLE_MASK, 0]
FORMS = [None, "rows", "records"]
FEASIBLE = abi.KG_DIAG_FEASIBLE
EXT = {"c5_64": (64, 16), "c5_200": (200, 70)}
CLUSTERS = list(ref.CLUSTERS) + list(EXT)


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def case(name):
    """(kg_config, nodes, pods, quotas, rsv, the oracle's status matrix) of one cluster; read-only."""
    if name in EXT:
        cfg, nodes, pods, quotas, rsv = synth.cluster5(*EXT[name], seed_config=12)
        kc = cfg.kg_config()
        ver = oracle_lib.ext_verify(kc, nodes, pods, quotas, rsv if kc.plugins & abi.KG_PLUGIN_RSV else None)
    else:
        cfg, nodes, pods = ref.CLUSTERS[name](synth)
        kc = cfg.kg_config()
        quotas = rsv = None
        ver = oracle_lib.eval_verify(kc, nodes, pods)
    for a in (ver.status, ver.total):
        a.setflags(write=False)
    return kc, nodes, pods, quotas, rsv, ver


@functools.lru_cache(maxsize=None)
def sets_of(name):
    kc, nodes, pods, quotas, rsv, ver = case(name)
    mask, pod_set, bits, kind = ref.kind_masks(ver.status, ver.total)
    for a in (mask, pod_set, bits, kind):
        a.setflags(write=False)
    return mask, pod_set, bits, kind


def make(ctx, name):
    kc, nodes, pods, quotas, rsv, ver = case(name)
    snap = engine.Snapshot(ctx, kc, nodes)
    if name in EXT:
        snap.upload_quotas(quotas)
        if kc.plugins & abi.KG_PLUGIN_RSV:
            snap.upload_reservations(rsv)
    return snap, engine.PodBatch(ctx, pods)


def expected(status, fail_mask):
    return nodesets.pack((status & np.uint32(fail_mask)) == 0)


def popcount(bits):
    return np.unpackbits(np.ascontiguousarray(bits, "<u4").view(np.uint8), axis=1).sum(axis=1).astype(np.uint32)


def set_form(monkeypatch, form):
    if form is None:
        monkeypatch.delenv("KG_FEASIBLE_FORM", raising=False)
    else:
        monkeypatch.setenv("KG_FEASIBLE_FORM", form)


def row_lists(n_pods):
    sub = np.random.default_rng(n_pods).permutation(n_pods)[:max(3, n_pods // 2)].astype(np.uint32)
    sub = np.concatenate([sub, sub[:1]])  # a shuffled subset with a repeat
    return [None, sub, np.array([5], np.uint32)]


# ---- 1. parity ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS, ids=["default", "rows", "records"])
@pytest.mark.parametrize("name", CLUSTERS)
def test_parity(ctx, monkeypatch, name, form):
    kc, nodes, pods, quotas, rsv, ver = case(name)
    status = ver.status
    # what the table in the docstring claims, as far as the tests lean on it
    feas = status == 0
    assert feas.any() and not feas.all(axis=1).any() and not (status & abi.KG_ST_UNSUPPORTED).any()
    set_form(monkeypatch, form)
    snap, batch = make(ctx, name)
    for fail_mask in MASKS:
        want = expected(status, fail_mask)
        for rows in row_lists(batch.n):
            got = engine.eval_feasible(snap, batch, rows, fail_mask)
            exp = want if rows is None else want[rows]
            assert got.dtype == np.uint32 and got.shape == exp.shape
            assert np.array_equal(got, exp), (hex(fail_mask), None if rows is None else len(rows),
                                              np.argwhere(got != exp)[:4])
    # fail_mask 0: every node bit, and nothing at or above n_nodes
    full = engine.eval_feasible(snap, batch, None, 0)
    assert np.array_equal(nodesets.to_mask(full, snap.n), np.ones((batch.n, snap.n), bool))
    if snap.n & 31:
        assert (full[:, -1] == np.uint32((1 << (snap.n & 31)) - 1)).all()
    # the masks ask different questions of these clusters
    assert not np.array_equal(expected(status, ALL), expected(status, abi.KG_ST_NRF_MASK))


# ---- 2. candidate node sets --------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS, ids=["default", "rows", "records"])
@pytest.mark.parametrize("name", ["small", "n129"])
def test_with_node_sets(ctx, monkeypatch, name, form):
    kc, nodes, pods, quotas, rsv, ver = case(name)
    mask, pod_set, bits, kind = sets_of(name)
    assert (kind == 3).any() and (kind == 6).any(), "the empty set and the explicit all-true set"
    set_form(monkeypatch, form)
    snap, batch = make(ctx, name)
    plain = engine.eval_feasible(snap, batch)
    batch.set_node_sets(pod_set, bits, snap.n)
    words = ref.expected_status(ver.status, mask)
    sub = np.array([9, 3, 3, batch.n - 1], np.uint32)
    for fail_mask in (ALL, EXCL, abi.KG_ST_NRF_MASK | EXCL):  # the excluded bit in the mask: excluded nodes are clear
        got = engine.eval_feasible(snap, batch, None, fail_mask)
        assert np.array_equal(got, expected(words, fail_mask)), hex(fail_mask)
        assert not (nodesets.to_mask(got, snap.n) & ~mask).any()
        assert np.array_equal(engine.eval_feasible(snap, batch, sub, fail_mask), expected(words, fail_mask)[sub])
    assert not engine.eval_feasible(snap, batch, None, ALL)[kind == 3].any(), "the empty set: a zero row"
    # the bit cleared from the mask: the bitmap without sets
    assert np.array_equal(engine.eval_feasible(snap, batch, None, ALL & ~EXCL), plain)
    assert np.array_equal(plain, expected(ver.status, ALL))
    batch.clear_node_sets()
    assert np.array_equal(engine.eval_feasible(snap, batch), plain)


# ---- 3. cross-checks ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "mixed", "c5_64", "c5_200"])
def test_counts_diagnose_and_select(ctx, name):
    kc, nodes, pods, quotas, rsv, ver = case(name)
    snap, batch = make(ctx, name)
    for fail_mask in MASKS:
        bits, cnt = engine.eval_feasible(snap, batch, None, fail_mask, counts=True)
        assert cnt.dtype == np.uint32 and cnt.shape == (batch.n,)
        assert np.array_equal(cnt, popcount(bits)), hex(fail_mask)
        assert np.array_equal(bits, expected(ver.status, fail_mask))
    bits, cnt = engine.eval_feasible(snap, batch, counts=True)
    assert np.array_equal(cnt, engine.eval_diagnose(snap, batch, first_plugin=False)[:, FEASIBLE])
    rows = np.array([7, 2, 2, 0], np.uint32)
    sub_bits, sub_cnt = engine.eval_feasible(snap, batch, rows, counts=True)
    assert np.array_equal(sub_bits, bits[rows]) and np.array_equal(sub_cnt, cnt[rows])
    # an empty bitmap is a pod without a host, and the reverse
    keys = engine.eval_select(snap, batch, 1)[:, 0]
    assert np.array_equal(cnt == 0, keys == 0) and (keys != 0).any()
    if name == "c5_64":
        empty = np.flatnonzero((ver.status != 0).all(axis=1))
        assert len(empty) == 2
        assert not bits[empty].any() and not cnt[empty].any() and bits[np.setdiff1d(np.arange(batch.n), empty)].any()


# ---- 4. round trip through the node sets -------------------------------------------------------------------------
def test_round_trip_through_node_sets(ctx):
    kc, nodes, pods, quotas, rsv, ver = case("small")
    snap, batch = make(ctx, "small")
    plain = {k: engine.eval_select(snap, batch, k) for k in (1, 3)}
    bits = engine.eval_feasible(snap, batch)
    batch.set_node_sets(np.arange(batch.n, dtype=np.int32), bits, snap.n)  # one set per pod: its feasible nodes
    for k in (1, 3):
        assert np.array_equal(engine.eval_select(snap, batch, k), plain[k]), k
        assert np.array_equal(plain[k], oracle_lib.select(kc, nodes, pods, k))


# ---- 5. no side effects ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "c5_200"])
def test_no_side_effects(ctx, name):
    kc, nodes, pods, quotas, rsv, ver = case(name)
    snap, batch = make(ctx, name)
    keys = engine.eval_select(snap, batch, 3)
    status = engine.result_status(batch)
    gen = snap.generation()
    engine.eval_feasible(snap, batch, None, abi.KG_ST_NRF_MASK, counts=True)
    engine.eval_feasible(snap, batch, [1, 0])
    assert np.array_equal(engine.result_keys(batch, 3), keys)
    assert np.array_equal(engine.result_status(batch), status)
    assert snap.generation() == gen
    if name in EXT:
        want = oracle_lib.ext_select(kc, nodes, pods, 3, quotas=quotas, rsv=rsv if kc.plugins & abi.KG_PLUGIN_RSV else None)
    else:
        want = oracle_lib.select(kc, nodes, pods, 3)
    assert np.array_equal(engine.eval_select(snap, batch, 3), want)


# ---- 6. arguments and refusals -----------------------------------------------------------------------------------
def test_arguments(ctx):
    kc, nodes, pods, quotas, rsv, ver = case("n129")
    snap, batch = make(ctx, "n129")
    L, P = ctx.L, C.POINTER(C.c_uint32)
    w = nodesets.words(snap.n)
    out = np.zeros((batch.n, w), np.uint32)
    cnt = np.zeros(batch.n, np.uint32)
    row0 = np.zeros(1, np.uint32)
    bad = [
        lambda: ctx.check(L.kg_eval_feasible(snap.h, batch.h, None, batch.n, ALL, None, None), "null output"),
        lambda: ctx.check(L.kg_eval_feasible(snap.h, batch.h, row0.ctypes.data_as(P), 1, ALL, None, cnt.ctypes.data_as(P)),
                          "null output, one row"),
        lambda: engine.eval_feasible(snap, batch, [batch.n]),
        lambda: engine.eval_feasible(snap, batch, [0, 0xFFFFFFFF]),
        lambda: ctx.check(L.kg_eval_feasible(snap.h, batch.h, None, batch.n - 1, ALL, out.ctypes.data_as(P), None), "n_rows"),
        lambda: ctx.check(L.kg_eval_feasible(snap.h, batch.h, None, 0, ALL, out.ctypes.data_as(P), None), "n_rows 0, no rows"),
    ]
    for call in bad:
        with pytest.raises(engine.EngineError) as ei:
            call()
        assert ei.value.status == abi.KG_INVALID_ARG
        assert "koordgpu" in str(ei.value)
    # n_rows == 0: KG_OK, nothing written, with or without an output
    guard = np.full(w + 1, 0xDEADBEEF, np.uint32)
    ctx.check(L.kg_eval_feasible(snap.h, batch.h, row0.ctypes.data_as(P), 0, ALL, guard.ctypes.data_as(P),
                                 guard[w:].ctypes.data_as(P)), "n_rows 0")
    ctx.check(L.kg_eval_feasible(snap.h, batch.h, row0.ctypes.data_as(P), 0, ALL, None, None), "n_rows 0, null output")
    assert (guard == 0xDEADBEEF).all()
    got = engine.eval_feasible(snap, batch, [], counts=True)
    assert got[0].shape == (0, w) and got[1].shape == (0,)
    # the context still works
    assert np.array_equal(engine.eval_feasible(snap, batch), expected(ver.status, ALL))


def test_snapshot_of_no_nodes(ctx):
    kc, nodes, pods, quotas, rsv, ver = case("n33")
    snap0 = engine.Snapshot(ctx, kc, abi.take(nodes, np.zeros(0, np.int64)))
    batch = engine.PodBatch(ctx, pods)
    L, P = ctx.L, C.POINTER(C.c_uint32)
    guard = np.full(4, 0xDEADBEEF, np.uint32)  # 0 words per row: nothing is written
    cnt = np.full(batch.n, 7, np.uint32)
    ctx.check(L.kg_eval_feasible(snap0.h, batch.h, None, batch.n, ALL, guard.ctypes.data_as(P), cnt.ctypes.data_as(P)),
              "0 nodes")
    assert (guard == 0xDEADBEEF).all() and not cnt.any()
    bits, cnt = engine.eval_feasible(snap0, batch, counts=True)
    assert bits.shape == (batch.n, 0) and not cnt.any()
    assert nodesets.to_mask(bits, 0).shape == (batch.n, 0)


def test_config5_snapshot_with_sets_is_refused(ctx):
    snap, batch = make(ctx, "c5_64")
    mask = np.ones((batch.n, snap.n), bool)
    mask[:, ::2] = False
    batch.set_node_sets(*nodesets.from_mask(mask), snap.n)
    with pytest.raises(engine.Unsupported):
        engine.eval_feasible(snap, batch)
    batch.clear_node_sets()
    assert np.array_equal(engine.eval_feasible(snap, batch), expected(case("c5_64")[5].status, ALL))


def test_node_count_mismatch_with_sets(ctx):
    kc, nodes, pods, quotas, rsv, ver = case("n129")
    mask, pod_set, bits, kind = sets_of("n129")
    snap, batch = make(ctx, "n129")
    wrong = nodesets.pack(np.zeros((len(bits), snap.n + 1), bool))
    batch.set_node_sets(pod_set, wrong, snap.n + 1)  # a bitmap over another node count: found by the evaluating call
    with pytest.raises(engine.EngineError) as e:
        engine.eval_feasible(snap, batch)
    assert e.value.status == abi.KG_INVALID_ARG


# ---- 7. regrow ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS, ids=["default", "rows", "records"])
def test_regrow(ctx, monkeypatch, form):
    kc, nodes, pods, quotas, rsv, ver = case("mixed")
    set_form(monkeypatch, form)
    snap, batch = make(ctx, "mixed")
    assert batch.n == 160
    want, wcnt = expected(ver.status, ALL), (ver.status == 0).sum(axis=1).astype(np.uint32)
    few = np.array([3, 159, 0, 77, 3, 12, 100, 41], np.uint32)
    for rows in (few, None, few[::-1].copy()):  # 8 rows, then 160 (the scratch grows), then 8 again
        bits, cnt = engine.eval_feasible(snap, batch, rows, counts=True)
        sel = slice(None) if rows is None else rows
        assert np.array_equal(bits, want[sel]) and np.array_equal(cnt, wcnt[sel])
