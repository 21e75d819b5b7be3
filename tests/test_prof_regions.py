"""The device-clock bracket of the one-launch top-1 select without same-address atomics (k_select_small's prof,
kg_kernels.hip; kg_ctx.d_prof, ensure_prof, prof_take and prof_drain in kg_runtime.cpp). A profiled launch
gets a region of the context's pool, one 16-byte pair {entry time, end time} per workgroup, written by plain stores; the
host keeps the workgroup count per pending launch and the drain folds each region (k_prof_fold, then the host over its
four words per launch): begin = the earliest entry, end = the latest end. The pool holds PROF_PAIRS pairs and the
launch table PROF_SLOTS launches; whichever fills first is drained by the select that finds it full. So the cases are about: a fold over the wrong extent (a neighbour's pairs, or
too few), a region that crosses the pool's end, a launch counted twice or not at all, a form whose workgroups do not all
store an end, and pairs that were not zeroed for the next launch.

No fixed time anywhere. A per-select bracket is compared with the bound-event figure (KG_PROFILE_BOUND_EVENTS=1) taken
in the same test on the same data. The event pair brackets the dispatch, which encloses every workgroup's entry and
end, so the clock figure cannot exceed it but for the variation between launches, and what the dispatch adds (launch
ramp and release) is less than the kernel itself: the two must agree within a factor of two either way, in every case
(test_device_clock_bracket.test_unit's criterion). A fold that took the latest entry or the earliest end, or ran over
too few pairs of a launch whose workgroups enter one after another, gives a fraction of the launch.

Snapshots are synth.small's nodes: 300, 600 and 4,096 / 4,097 of them, and three subsets of the 300 for the launches of
one, two and eight workgroups (a chunk holds at most 64 records). Batches are 37 and 145 distinct fast pods. Keys are
checked against the oracle in every case. KG_SMALL_ALLOW_BIG=1 keeps the F_BIG gate out of the way."""
import numpy as np
import pytest

import oracle_lib
from koordinator_amd import abi, synth
from test_small_fused import n_chunks, small_cluster
from test_small_lane_results import shuffled37
from test_small_select import fast_distinct

CUS = 256                # compute units of an MI355X
PROF_SLOTS = 256         # kg_ctx::PROF_SLOTS, kg_runtime.cpp
PROF_PAIRS = 65536       # kg_ctx::PROF_PAIRS
SMALL_MAX_CHUNKS = 4096  # kg_kernels.h
ENV = ("KG_NO_SMALL_SELECT", "KG_SMALL_ROW_RESULTS", "KG_SMALL_FINISHER", "KG_NO_POD_DEDUP", "KG_SMALL_REPLICAS",
       "KG_SMALL_PHASES", "KG_PROFILE_BOUND_EVENTS", "KG_NO_SMALL_FUSED_FINISH", "KG_SMALL_CHUNKS")
# workgroups -> (records of class 0, records of class 1, KG_SMALL_CHUNKS)
FEW = {1: (5, 0, "64,64,1"), 2: (5, 5, "64,64,1"), 8: (32, 32, "8,8,1")}
FORMS = {"acc": None, "finisher": "KG_SMALL_FINISHER", "rows": "KG_SMALL_ROW_RESULTS"}


def few_nodes(count):
    """A subset of the 300 nodes that the geometry FEW[count] walks in `count` workgroups."""
    kc, nodes = small_cluster()
    single = nodes["numa_policy"] == abi.KG_NUMA_SINGLE_NODE
    n0, n1, _ = FEW[count]
    return kc, abi.take(nodes, np.concatenate([np.flatnonzero(~single)[:n0], np.flatnonzero(single)[:n1]]))


_nodes = {}


def synth_nodes(n):
    """The first n of synth.small(4097, 64)'s nodes (300: small_cluster's own), made once."""
    if n == 300:
        return small_cluster()
    if "big" not in _nodes:
        cfg, nodes, _ = synth.small(SMALL_MAX_CHUNKS + 1, 64, seed=7)
        _nodes["big"] = (cfg.kg_config(), nodes)
    kc, nodes = _nodes["big"]
    return kc, abi.take(nodes, np.arange(n))


_want = {}


def oracle_keys(tag, kc, nodes, pods):
    """The oracle's top-1 keys, computed once per tag and left unchanged."""
    if tag not in _want:
        _want[tag] = oracle_lib.select(kc, nodes, pods, 1)
        _want[tag].setflags(write=False)
    return _want[tag]


def test_inputs():
    """CPU side: the subsets give the workgroup counts they are named for, one record per workgroup gives more
    workgroups than compute units on 600 nodes and exactly the limit and one more on 4,096 and 4,097, and the bursts
    fill the pool before the launch table or the table before the pool."""
    for count, (n0, n1, chunks) in FEW.items():
        _, sub = few_nodes(count)
        c0, c1, _ = (int(v) for v in chunks.split(","))
        assert abi.table_len(sub) == n0 + n1 and n_chunks(sub, c0, c1) == count
    for n in (600, SMALL_MAX_CHUNKS, SMALL_MAX_CHUNKS + 1):
        assert n_chunks(synth_nodes(n)[1], 1, 1) == n
    assert 600 > CUS and PROF_PAIRS % 600 != 0 and PROF_PAIRS // 600 < 120 < PROF_SLOTS
    assert PROF_PAIRS // SMALL_MAX_CHUNKS + 5 < PROF_SLOTS
    kc, nodes = small_cluster()
    assert (PROF_SLOTS + 3) * n_chunks(nodes, 8, 8) < PROF_PAIRS


@pytest.fixture(scope="module")
def gpu():
    from koordinator_amd import engine
    ctx = engine.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("KG_SMALL_ALLOW_BIG", "1")


def profiled(ctx, snap, batch, n):
    """n async selects with profiling on and one read at the end: (bracket ms, launches)."""
    from koordinator_amd import engine
    ctx.sync()
    ctx.profile(True)
    try:
        ctx.profile_read(reset=True)
        for _ in range(n):
            engine.eval_select_async(snap, batch, 1)
        return ctx.profile_read(reset=True)
    finally:
        ctx.profile(False)


def check_bracket(ctx, snap, batch, monkeypatch, n, want, tag):
    """n selects with the device-clock bracket and n with the bound pair: n launches counted each time, the clock
    figure between half and twice the event figure, keys the oracle's."""
    from koordinator_amd import engine
    for _ in range(2):
        engine.eval_select_async(snap, batch, 1)
    ms_clock, launches = profiled(ctx, snap, batch, n)
    assert launches == n, (tag, launches)
    keys = engine.result_keys(batch, 1)
    bad = np.flatnonzero((keys != want).any(axis=1))
    assert not len(bad), (tag, "keys differ from the oracle", bad[:8], keys[bad[:8], 0], want[bad[:8], 0])
    monkeypatch.setenv("KG_PROFILE_BOUND_EVENTS", "1")
    ms_events, launches = profiled(ctx, snap, batch, n)
    monkeypatch.delenv("KG_PROFILE_BOUND_EVENTS")
    assert launches == n, (tag, "bound events", launches)
    print(f"{tag}: device clock {ms_clock / n:.5f} ms per select, bound events {ms_events / n:.5f} ms")
    assert 0 < 0.5 * ms_events < ms_clock < 2.0 * ms_events, (tag, ms_clock / n, ms_events / n)
    assert ctx.profile_read() == (0.0, 0)
    return ms_clock / n


@pytest.mark.gpu
@pytest.mark.parametrize("count", list(FEW))
def test_workgroup_counts(gpu, monkeypatch, count):
    """Launches of one, two and eight workgroups: the fold runs over exactly that many pairs."""
    from koordinator_amd import engine
    ctx = gpu
    kc, sub = few_nodes(count)
    pods = shuffled37()
    snap = engine.Snapshot(ctx, kc, sub)
    batch = engine.PodBatch(ctx, pods)
    monkeypatch.setenv("KG_SMALL_CHUNKS", FEW[count][2])
    try:
        assert batch.fast_lanes(snap) == 37
        check_bracket(ctx, snap, batch, monkeypatch, 9, oracle_keys(("few", count), kc, sub, pods), f"{count} workgroups")
    finally:
        batch.close()
        snap.close()


@pytest.mark.gpu
def test_more_workgroups_than_compute_units(gpu, monkeypatch):
    """KG_SMALL_CHUNKS=1,1,1 on 600 nodes: 600 workgroups, some enter when others have ended, so the earliest entry
    and the latest end belong to different workgroups. 120 launches do not fit in the pool (65,536 is no multiple of
    600): the launch whose region would cross the pool's end drains first."""
    from koordinator_amd import engine
    ctx = gpu
    kc, nodes = synth_nodes(600)
    pods = shuffled37()
    snap = engine.Snapshot(ctx, kc, nodes)
    batch = engine.PodBatch(ctx, pods)
    monkeypatch.setenv("KG_SMALL_CHUNKS", "1,1,1")
    try:
        assert batch.fast_lanes(snap) == 37
        check_bracket(ctx, snap, batch, monkeypatch, 120, oracle_keys(600, kc, nodes, pods), "600 workgroups")
    finally:
        batch.close()
        snap.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n_nodes", [SMALL_MAX_CHUNKS, SMALL_MAX_CHUNKS + 1])
def test_chunk_limit(gpu, monkeypatch, n_nodes):
    """One record per workgroup on 4,096 nodes: the largest grid of the one-launch path, sixteen regions fill the pool
    and 21 launches drain it in the loop. On 4,097 nodes the select leaves the one-launch path and is still counted,
    through its event pair: both figures are then the same bracket."""
    from koordinator_amd import engine
    ctx = gpu
    kc, nodes = synth_nodes(n_nodes)
    pods = shuffled37()
    snap = engine.Snapshot(ctx, kc, nodes)
    batch = engine.PodBatch(ctx, pods)
    monkeypatch.setenv("KG_SMALL_CHUNKS", "1,1,1")
    try:
        assert batch.fast_lanes(snap) == 37
        n = PROF_PAIRS // SMALL_MAX_CHUNKS + 5
        check_bracket(ctx, snap, batch, monkeypatch, n, oracle_keys(n_nodes, kc, nodes, pods), f"{n_nodes} nodes")
    finally:
        batch.close()
        snap.close()


@pytest.mark.gpu
def test_more_selects_than_table_entries(gpu, monkeypatch):
    """PROF_SLOTS + 3 profiled selects and no read in between: the launch table fills before the pool, the select that
    finds it full drains it, and the count is the burst's."""
    from koordinator_amd import engine
    ctx = gpu
    kc, nodes = small_cluster()
    pods = shuffled37()
    snap = engine.Snapshot(ctx, kc, nodes)
    batch = engine.PodBatch(ctx, pods)
    monkeypatch.setenv("KG_SMALL_CHUNKS", "8,8,1")
    try:
        check_bracket(ctx, snap, batch, monkeypatch, PROF_SLOTS + 3, oracle_keys(300, kc, nodes, pods), "table full")
    finally:
        batch.close()
        snap.close()


@pytest.mark.gpu
@pytest.mark.parametrize("chunks", [None, "1,1,1"])
@pytest.mark.parametrize("form", list(FORMS))
def test_result_forms(gpu, monkeypatch, form, chunks):
    """The form without a finisher (every workgroup stores an end) and the two finisher forms (the finishing workgroup
    alone does), at the default geometry and with more workgroups than compute units."""
    from koordinator_amd import engine
    ctx = gpu
    kc, nodes = small_cluster()
    pods = fast_distinct(145)
    snap = engine.Snapshot(ctx, kc, nodes)
    batch = engine.PodBatch(ctx, pods)
    if FORMS[form]:
        monkeypatch.setenv(FORMS[form], "1")
    if chunks:
        monkeypatch.setenv("KG_SMALL_CHUNKS", chunks)
    try:
        assert batch.fast_lanes(snap) == 145
        check_bracket(ctx, snap, batch, monkeypatch, 12, oracle_keys((300, 145), kc, nodes, pods), f"{form} {chunks}")
    finally:
        batch.close()
        snap.close()


@pytest.mark.gpu
def test_reads(gpu, monkeypatch):
    """profile_read twice without a reset gives the same totals (the first drained the pool, the second finds nothing
    pending and adds nothing); more selects add to them; a select after profile(False) leaves nothing pending."""
    from koordinator_amd import engine
    ctx = gpu
    kc, nodes = small_cluster()
    pods = shuffled37()
    snap = engine.Snapshot(ctx, kc, nodes)
    batch = engine.PodBatch(ctx, pods)
    try:
        ctx.profile(True)
        try:
            ctx.profile_read(reset=True)
            for _ in range(5):
                engine.eval_select_async(snap, batch, 1)
            first = ctx.profile_read()
            assert first[1] == 5 and first[0] > 0
            assert ctx.profile_read() == first
            for _ in range(3):
                engine.eval_select_async(snap, batch, 1)
            more = ctx.profile_read()
            assert more[1] == 8 and more[0] > first[0]
            assert ctx.profile_read(reset=True) == more
            assert ctx.profile_read() == (0.0, 0)
        finally:
            ctx.profile(False)
        for _ in range(3):
            engine.eval_select_async(snap, batch, 1)
        ctx.sync()
        ctx.profile(True)
        try:
            assert ctx.profile_read() == (0.0, 0)
            engine.eval_select_async(snap, batch, 1)
            ms, launches = ctx.profile_read(reset=True)
            assert launches == 1 and ms > 0
        finally:
            ctx.profile(False)
        assert np.array_equal(engine.result_keys(batch, 1), oracle_keys(300, kc, nodes, pods))
    finally:
        batch.close()
        snap.close()


@pytest.mark.gpu
def test_two_batches_interleaved(gpu, monkeypatch):
    """Two batches of 37 and 145 lanes on two snapshots of 300 and 600 nodes (other workgroup counts), selects
    alternating on one context: neighbouring regions of the pool have different lengths. The total is the sum of what
    each batch measures alone, within the factor of the bracket check, and each batch reads its own keys."""
    from koordinator_amd import engine
    ctx = gpu
    kc, nodes = small_cluster()
    kc6, nodes6 = synth_nodes(600)
    pods_a, pods_b = shuffled37(), fast_distinct(145)
    snap_a, snap_b = engine.Snapshot(ctx, kc, nodes), engine.Snapshot(ctx, kc6, nodes6)
    a, b = engine.PodBatch(ctx, pods_a), engine.PodBatch(ctx, pods_b)
    n = 10
    try:
        want_a, want_b = oracle_keys(300, kc, nodes, pods_a), oracle_keys((600, 145), kc6, nodes6, pods_b)
        per_a = check_bracket(ctx, snap_a, a, monkeypatch, n, want_a, "batch a alone")
        per_b = check_bracket(ctx, snap_b, b, monkeypatch, n, want_b, "batch b alone")
        ctx.profile(True)
        try:
            ctx.profile_read(reset=True)
            for i in range(n):
                engine.eval_select_async(snap_a, a, 1)
                engine.eval_select_async(snap_b, b, 1)
                if i == n // 2:
                    assert ctx.profile_read()[1] == 2 * i + 2
            ms, launches = ctx.profile_read(reset=True)
        finally:
            ctx.profile(False)
        print(f"interleaved: {ms / n:.5f} ms per pair of selects, alone {per_a:.5f} + {per_b:.5f}")
        assert launches == 2 * n
        assert 0.5 * (per_a + per_b) < ms / n < 2.0 * (per_a + per_b)
        assert np.array_equal(engine.result_keys(a, 1), want_a)
        assert np.array_equal(engine.result_keys(b, 1), want_b)
    finally:
        b.close()
        a.close()
        snap_b.close()
        snap_a.close()
