"""The profile bracket of the one-pod-block top-1 select (kg_profile_enable / kg_profile_read around select_local's small
path, kg_runtime.cpp): with profiling on the launch carries the pooled event pair itself (hipExtLaunchKernelGGL: start
event on k_select_small, stop event on the kernel that ends the step) instead of two hipEventRecord calls around it.
Every other bracket (the general select here) still records its pair, and both kinds share one pool.

The snapshot is test_small_select.test_path_is_taken's: test_pod_dedup's mixed cluster thinned to the records that are
neither F_BIG nor BestEffort (both storage classes, the F_BIG gate passes by itself). The batch is 145 distinct fast
pods tiled to 435 rows: three waves of lanes, the last partly idle, every row served through lane_of. At the default
geometry that is dozens of chunks and five copies of the lanes per workgroup (the 1,024-thread variant); the
KG_SMALL_CHUNKS forms set two copies (the 512-thread variant) and five with other chunk lengths.

Checked: results do not depend on profiling (keys and status, bit for bit, and against the oracle) in each form; the
counters count one bracket per select, none with profiling off, from zero after a reset (pooled pairs reused); the
bracket is a device time (below the wall-clock time per step of the same loop; the default form's below the general
path's); small and general selects interleaved on one context count and compute right."""
import time

import numpy as np
import pytest

import oracle_lib
from koordinator_amd import abi
from test_pod_dedup import cluster, distinct_rows
from test_small_select import fast_distinct, is_big

LANES, ROWS = 145, 435
FORMS = {
    "default": {},
    "two_launch": {"KG_NO_SMALL_FUSED_FINISH": "1"},
    "general": {"KG_NO_SMALL_SELECT": "1"},
    "chunks_2_copies": {"KG_SMALL_CHUNKS": "8,6,2"},  # 2 x 192 threads: the 512-thread variant
    "chunks_5_copies": {"KG_SMALL_CHUNKS": "7,5,5"},  # 5 x 192 threads: the 1,024-thread variant
}
COUNTED = ["default", "two_launch", "general"]


def inputs():
    kc, nodes, _ = cluster()
    sub = abi.take(nodes, np.flatnonzero(~is_big(nodes) & (nodes["numa_policy"] != abi.KG_NUMA_BEST_EFFORT)))
    pods = abi.take(fast_distinct(LANES), np.arange(ROWS) % LANES)
    return kc, sub, pods


_want = {}


def oracle_keys(kc, nodes, pods, k):
    """The oracle's top-k keys, computed once per k and left unchanged."""
    if k not in _want:
        _want[k] = oracle_lib.select(kc, nodes, pods, k)
        _want[k].setflags(write=False)
    return _want[k]


def test_inputs():
    """CPU side: the snapshot holds both storage classes and no F_BIG record, in several chunks of the default geometry
    (at least 8 records each) and of the KG_SMALL_CHUNKS forms; the batch has 145 distinct rows, all feasible somewhere."""
    kc, sub, pods = inputs()
    single = sub["numa_policy"] == abi.KG_NUMA_SINGLE_NODE
    assert single.sum() > 64 and (~single).sum() > 64 and not is_big(sub).any()
    assert abi.table_len(pods) == ROWS and distinct_rows(pods) == LANES
    assert (oracle_keys(kc, sub, pods, 1) != 0).any()


@pytest.fixture(scope="module")
def gpu():
    from koordinator_amd import engine
    kc, sub, pods = inputs()
    ctx = engine.Context(0)
    snap = engine.Snapshot(ctx, kc, sub)
    batch = engine.PodBatch(ctx, pods)
    assert batch.select_lanes() == (LANES, LANES)
    yield ctx, snap, batch, kc, sub, pods
    ctx.close()


def set_form(monkeypatch, form):
    for name in ("KG_NO_SMALL_FUSED_FINISH", "KG_NO_SMALL_SELECT", "KG_SMALL_CHUNKS", "KG_SMALL_REPLICAS", "KG_SMALL_ALLOW_BIG"):
        monkeypatch.delenv(name, raising=False)
    for name, value in FORMS[form].items():
        monkeypatch.setenv(name, value)


def profiled_loop(ctx, snap, batch, n, k=1):
    """n async selects and one sync with profiling on, after a warm-up: (bracket ms, launches, wall-clock ms), totals."""
    from koordinator_amd import engine
    for _ in range(3):
        engine.eval_select_async(snap, batch, k)
    ctx.sync()
    ctx.profile(True)
    try:
        ctx.profile_read(reset=True)
        t0 = time.perf_counter()
        for _ in range(n):
            engine.eval_select_async(snap, batch, k)
        ctx.sync()
        wall = (time.perf_counter() - t0) * 1e3
        ms, launches = ctx.profile_read(reset=True)
    finally:
        ctx.profile(False)
    return ms, launches, wall


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(FORMS))
def test_results_do_not_depend_on_profiling(gpu, monkeypatch, form):
    from koordinator_amd import engine
    ctx, snap, batch, kc, sub, pods = gpu
    set_form(monkeypatch, form)
    want = oracle_keys(kc, sub, pods, 1)
    keys_off = engine.eval_select(snap, batch, 1)
    status_off = engine.result_status(batch)
    ctx.profile(True)
    try:
        ctx.profile_read(reset=True)
        keys_on = engine.eval_select(snap, batch, 1)
        status_on = engine.result_status(batch)
        keys_on2 = engine.eval_select(snap, batch, 1)  # a second bracket while the first pair is still live
        status_on2 = engine.result_status(batch)
        ms, launches = ctx.profile_read(reset=True)
    finally:
        ctx.profile(False)
    assert launches == 2 and ms > 0
    for keys, status in ((keys_on, status_on), (keys_on2, status_on2)):
        bad = np.flatnonzero((keys != keys_off).any(axis=1))
        assert not len(bad), ("keys differ with profiling on", bad[:8], keys[bad[:8], 0], keys_off[bad[:8], 0])
        assert np.array_equal(status, status_off), ("status differs with profiling on", np.flatnonzero(status != status_off)[:8])
    bad = np.flatnonzero((keys_off != want).any(axis=1))
    assert not len(bad), ("keys differ from the oracle", bad[:8])
    # the select after profiling is switched off again
    assert np.array_equal(engine.eval_select(snap, batch, 1), keys_off)
    assert np.array_equal(engine.result_status(batch), status_off)
    assert ctx.profile_read(reset=True)[1] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("form", COUNTED)
def test_counting(gpu, monkeypatch, form):
    """One bracket per select; none with profiling off; a second round after reset=True counts from zero, on the pairs
    that the first round returned to the pool."""
    from koordinator_amd import engine
    ctx, snap, batch, kc, sub, pods = gpu
    set_form(monkeypatch, form)
    n = 12
    ms, launches, _ = profiled_loop(ctx, snap, batch, n)
    assert launches == n and ms > 0
    for _ in range(4):
        engine.eval_select_async(snap, batch, 1)
    ctx.sync()
    ms_off, launches_off = ctx.profile_read(reset=True)
    assert launches_off == 0 and ms_off == 0
    ms2, launches2, _ = profiled_loop(ctx, snap, batch, n - 5)
    assert launches2 == n - 5 and ms2 > 0
    # without a reset the counters add up
    ctx.profile(True)
    try:
        engine.eval_select_async(snap, batch, 1)
        assert ctx.profile_read()[1] == 1
        engine.eval_select_async(snap, batch, 1)
        ms3, launches3 = ctx.profile_read(reset=True)
    finally:
        ctx.profile(False)
    assert launches3 == 2 and ms3 > 0
    assert np.array_equal(engine.result_keys(batch, 1), oracle_keys(kc, sub, pods, 1))


@pytest.mark.gpu
def test_bracket_is_a_device_time(gpu, monkeypatch):
    """The bracket per select is below the wall-clock time per step of the loop it was taken in, in each form, and the
    default form's is below the general path's on the same data (test_small_select.test_path_is_taken's criterion: a
    select that fell back to the general path would measure the same). The figures are printed; no absolute time."""
    ctx, snap, batch, kc, sub, pods = gpu
    n = 40
    per = {}
    for form in COUNTED:
        set_form(monkeypatch, form)
        ms, launches, wall = profiled_loop(ctx, snap, batch, n)
        assert launches == n
        per[form] = (ms / n, wall / n)
        print(f"{form}: bracket {ms / n:.5f} ms per select, wall clock {wall / n:.5f} ms per step")
    for form, (bracket, wall) in per.items():
        assert 0 < bracket < wall, (form, bracket, wall)
    assert per["default"][0] < per["general"][0]


@pytest.mark.gpu
def test_interleaving(gpu, monkeypatch):
    """A small select (pair bound to its launch), a general top-3 select (pair recorded around it) and a small select
    again on one context, then the same once more on the pooled pairs: three brackets each time, every key table equal
    to the oracle's."""
    from koordinator_amd import engine
    ctx, snap, batch, kc, sub, pods = gpu
    set_form(monkeypatch, "default")
    want1, want3 = oracle_keys(kc, sub, pods, 1), oracle_keys(kc, sub, pods, 3)
    ctx.profile(True)
    try:
        ctx.profile_read(reset=True)
        for _ in range(2):
            first = engine.eval_select(snap, batch, 1)
            middle = engine.eval_select(snap, batch, 3)
            last = engine.eval_select(snap, batch, 1)
            ms, launches = ctx.profile_read(reset=True)
            assert launches == 3 and ms > 0
            assert np.array_equal(first, want1) and np.array_equal(last, want1)
            bad = np.flatnonzero((middle != want3).any(axis=1))
            assert not len(bad), ("top-3 keys differ from the oracle", bad[:8])
    finally:
        ctx.profile(False)
