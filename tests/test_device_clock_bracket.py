"""The profile bracket of the one-launch top-1 select, taken inside the launch (k_select_small's prof, kg_kernels.hip;
select_local's small path and kg_profile_read, kg_runtime.cpp): with profiling on the kernel times itself
with the device's wall clock. Thread 0 of every workgroup folds the complement of its entry time into a begin word on
the ticket's line, the finisher takes the word back to zero and adds end - begin to a context-level tick sum, and
kg_profile_read converts the ticks by hipDeviceAttributeWallClockRate. The launch carries no event pair.
KG_PROFILE_BOUND_EVENTS=1 keeps the event pair bound to the launch, the two-launch form always has it.

Inputs are test_profile_bracket's: the mixed cluster thinned to the records that are neither F_BIG nor BestEffort, 145
distinct fast pods tiled to 435 rows; also 64 and 256 lanes on the same snapshot, five records of one class (one
workgroup: first and finisher at once) and one record per workgroup (more workgroups than the device has compute units).

Checked: keys and status do not depend on the bracket (bit for bit, and against the oracle); the counters count one
bracket per select whatever the mix of brackets; no begin word survives a launch (every single bracket lies below the
wall-clock time of its own select: a begin word left by an earlier launch would give at least the time since that
launch); the device-clock bracket and the bound pair's agree within a factor of two either way (the unit: a kHz / Hz
or complement error is off by orders of magnitude). No absolute time."""
import time

import numpy as np
import pytest

import oracle_lib
from koordinator_amd import abi
from test_pod_dedup import distinct_rows
from test_profile_bracket import LANES, ROWS, inputs, profiled_loop
from test_small_select import fast_distinct, is_big

CUS = 256  # compute units of an MI355X
SETTINGS = {
    "off": (False, {}),
    "clock": (True, {}),
    "events": (True, {"KG_PROFILE_BOUND_EVENTS": "1"}),
    "clock_512": (True, {"KG_SMALL_CHUNKS": "8,6,2"}),  # 2 copies of the lanes: the 512-thread variant
}
ENV = ("KG_NO_SMALL_FUSED_FINISH", "KG_NO_SMALL_SELECT", "KG_SMALL_CHUNKS", "KG_SMALL_REPLICAS", "KG_SMALL_ALLOW_BIG",
       "KG_PROFILE_BOUND_EVENTS", "KG_SMALL_PHASES")


def tiled(lanes):
    return abi.take(fast_distinct(lanes), np.arange(3 * lanes) % lanes)


def one_class_five(sub):
    """Five records of storage class 0 (no SingleNUMANode policy): one chunk at any geometry."""
    return abi.take(sub, np.flatnonzero(sub["numa_policy"] != abi.KG_NUMA_SINGLE_NODE)[:5])


_want = {}


def oracle_keys(name, kc, nodes, pods):
    """The oracle's top-1 keys, computed once per case and left unchanged."""
    if name not in _want:
        _want[name] = oracle_lib.select(kc, nodes, pods, 1)
        _want[name].setflags(write=False)
    return _want[name]


def clear_env(monkeypatch, env=None):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    for name, value in (env or {}).items():
        monkeypatch.setenv(name, value)


def test_inputs():
    """CPU side: both storage classes and no F_BIG record; 145 distinct rows in 435; the 64- and 256-lane batches are
    distinct fast pods, three rows per lane; one record per workgroup gives more workgroups than compute units; the
    five-record snapshot is of one class and some pod fits one of its nodes."""
    kc, sub, pods = inputs()
    single = sub["numa_policy"] == abi.KG_NUMA_SINGLE_NODE
    assert single.sum() > 64 and (~single).sum() > 64 and not is_big(sub).any()
    assert abi.table_len(pods) == ROWS and distinct_rows(pods) == LANES
    for lanes in (64, 256):
        t = tiled(lanes)
        assert abi.table_len(t) == 3 * lanes and distinct_rows(t) == lanes
    assert abi.table_len(sub) > CUS  # KG_SMALL_CHUNKS="1,1,1": one workgroup per record
    five = one_class_five(sub)
    assert abi.table_len(five) == 5 and not (five["numa_policy"] == abi.KG_NUMA_SINGLE_NODE).any()
    assert (oracle_keys("five", kc, five, pods) != 0).any()
    assert (oracle_keys(LANES, kc, sub, pods) != 0).any()


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


def select_in_settings(ctx, snap, batch, monkeypatch, want):
    """Keys and status of the default form in the four settings: all equal to the first and to the oracle's keys."""
    from koordinator_amd import engine
    got = {}
    for name, (profiling, env) in SETTINGS.items():
        clear_env(monkeypatch, env)
        ctx.profile(profiling)
        try:
            ctx.profile_read(reset=True)
            keys = engine.eval_select(snap, batch, 1)
            status = engine.result_status(batch)
            keys2 = engine.eval_select(snap, batch, 1)  # the begin word of the first launch is gone
            ms, launches = ctx.profile_read(reset=True)
        finally:
            ctx.profile(False)
        assert launches == (2 if profiling else 0) and (ms > 0) == profiling, (name, ms, launches)
        assert np.array_equal(keys, keys2), name
        got[name] = (keys, status)
    keys_off, status_off = got["off"]
    bad = np.flatnonzero((keys_off != want).any(axis=1))
    assert not len(bad), ("keys differ from the oracle", bad[:8])
    for name, (keys, status) in got.items():
        bad = np.flatnonzero((keys != keys_off).any(axis=1))
        assert not len(bad), (name, "keys differ from profiling off", bad[:8], keys[bad[:8], 0], keys_off[bad[:8], 0])
        assert np.array_equal(status, status_off), (name, "status differs", np.flatnonzero(status != status_off)[:8])


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [LANES, 64, 256])
def test_results(gpu, monkeypatch, lanes):
    from koordinator_amd import engine
    ctx, snap, batch, kc, sub, pods = gpu
    if lanes == LANES:
        select_in_settings(ctx, snap, batch, monkeypatch, oracle_keys(LANES, kc, sub, pods))
        return
    other = tiled(lanes)
    b = engine.PodBatch(ctx, other)
    try:
        assert b.select_lanes() == (lanes, lanes)
        select_in_settings(ctx, snap, b, monkeypatch, oracle_keys(lanes, kc, sub, other))
    finally:
        b.close()


@pytest.mark.gpu
def test_one_workgroup(gpu, monkeypatch):
    """Five records of one class: the only workgroup is first and finisher at once."""
    from koordinator_amd import engine
    ctx, _, batch, kc, sub, pods = gpu
    five = one_class_five(sub)
    snap = engine.Snapshot(ctx, kc, five)
    try:
        select_in_settings(ctx, snap, batch, monkeypatch, oracle_keys("five", kc, five, pods))
    finally:
        snap.close()


@pytest.mark.gpu
def test_counting(gpu, monkeypatch):
    """12 async selects, then profile_read without a sync of the caller's: 12 launches. Then one-launch selects (device
    clock), a top-3 general select (recorded pair), a two-launch select and a one-launch select with the bound pair,
    interleaved: the count is the sum, from zero after reset=True. With profiling off nothing is counted."""
    from koordinator_amd import engine
    ctx, snap, batch, kc, sub, pods = gpu
    clear_env(monkeypatch)
    want = oracle_keys(LANES, kc, sub, pods)
    ctx.profile(True)
    try:
        ctx.profile_read(reset=True)
        for _ in range(12):
            engine.eval_select_async(snap, batch, 1)
        ms, launches = ctx.profile_read(reset=True)
        assert launches == 12 and ms > 0
        assert ctx.profile_read() == (0.0, 0)
        n = 0
        for round_ in range(2):
            for _ in range(2):
                engine.eval_select_async(snap, batch, 1)
            engine.eval_select_async(snap, batch, 3)
            engine.eval_select_async(snap, batch, 1)
            monkeypatch.setenv("KG_NO_SMALL_FUSED_FINISH", "1")
            engine.eval_select_async(snap, batch, 1)
            monkeypatch.delenv("KG_NO_SMALL_FUSED_FINISH")
            monkeypatch.setenv("KG_PROFILE_BOUND_EVENTS", "1")
            engine.eval_select_async(snap, batch, 1)
            monkeypatch.delenv("KG_PROFILE_BOUND_EVENTS")
            engine.eval_select_async(snap, batch, 1)
            n += 7
            if round_ == 0:  # a read in between does not reset
                ms1, launches1 = ctx.profile_read()
                assert launches1 == 7 and ms1 > 0
        ms, launches = ctx.profile_read(reset=True)
        assert launches == n and ms > ms1
        assert np.array_equal(engine.result_keys(batch, 1), want)
    finally:
        ctx.profile(False)
    for _ in range(4):
        engine.eval_select_async(snap, batch, 1)
    ctx.sync()
    assert ctx.profile_read(reset=True) == (0.0, 0)


def timed_select(ctx, snap, batch):
    """One synchronised select with profiling on: (keys, bracket ms, wall-clock ms)."""
    from koordinator_amd import engine
    ctx.sync()
    ctx.profile(True)
    try:
        ctx.profile_read(reset=True)
        t0 = time.perf_counter()
        engine.eval_select_async(snap, batch, 1)
        ctx.sync()
        wall = (time.perf_counter() - t0) * 1e3
        ms, launches = ctx.profile_read(reset=True)
    finally:
        ctx.profile(False)
    assert launches == 1
    return engine.result_keys(batch, 1), ms, wall


@pytest.mark.gpu
def test_zero_state(gpu, monkeypatch):
    """Profiling on and off in turn, chunk and replica counts changing from call to call (test_small_fused's
    test_leftover_state), a read after every synchronised select: each bracket is positive and below the wall-clock
    time of its own select, and every key table is the oracle's."""
    from koordinator_amd import engine
    ctx, snap, batch, kc, sub, pods = gpu
    clear_env(monkeypatch)
    want = oracle_keys(LANES, kc, sub, pods)
    for _ in range(3):
        engine.eval_select_async(snap, batch, 1)
    ctx.sync()
    for chunks, replicas in ((None, None), ("8,8,1", "3"), ("7,5,2", "4000"), ("64,64,5", "1"), ("8,8,1", "2"), (None, None)):
        clear_env(monkeypatch, {k: v for k, v in (("KG_SMALL_CHUNKS", chunks), ("KG_SMALL_REPLICAS", replicas)) if v})
        for _ in range(2):
            keys, ms, wall = timed_select(ctx, snap, batch)
            print(f"chunks {chunks} replicas {replicas}: bracket {ms:.5f} ms, wall clock {wall:.5f} ms")
            assert np.array_equal(keys, want), (chunks, replicas)
            assert 0 < ms < wall, (chunks, replicas, ms, wall)
            # profiling off in between: a plain launch on the same accumulator buffer
            assert np.array_equal(engine.eval_select(snap, batch, 1), want), (chunks, replicas)
            assert ctx.profile_read(reset=True) == (0.0, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("chunks", ["1,1,1", "1,1,5"])
def test_more_workgroups_than_compute_units(gpu, monkeypatch, chunks):
    """One record per workgroup: more workgroups than compute units, so some start when others have ended."""
    ctx, snap, batch, kc, sub, pods = gpu
    assert snap.n > CUS
    clear_env(monkeypatch, {"KG_SMALL_CHUNKS": chunks})
    want = oracle_keys(LANES, kc, sub, pods)
    for _ in range(3):
        keys, ms, wall = timed_select(ctx, snap, batch)
        print(f"chunks {chunks}: bracket {ms:.5f} ms, wall clock {wall:.5f} ms")
        bad = np.flatnonzero((keys != want).any(axis=1))
        assert not len(bad), ("keys differ from the oracle", bad[:8])
        assert 0 < ms < wall, (ms, wall)


@pytest.mark.gpu
def test_unit(gpu, monkeypatch):
    """40 selects with the device-clock bracket and 40 with the bound pair, one process: per select they agree within a
    factor of two either way."""
    ctx, snap, batch, kc, sub, pods = gpu
    n = 40
    clear_env(monkeypatch)
    ms_clock, launches, wall_clock = profiled_loop(ctx, snap, batch, n)
    assert launches == n
    clear_env(monkeypatch, {"KG_PROFILE_BOUND_EVENTS": "1"})
    ms_events, launches, wall_events = profiled_loop(ctx, snap, batch, n)
    assert launches == n
    print(f"device clock: bracket {ms_clock / n:.5f} ms per select, wall clock {wall_clock / n:.5f} ms per step")
    print(f"bound events: bracket {ms_events / n:.5f} ms per select, wall clock {wall_events / n:.5f} ms per step")
    assert ms_clock > 0 and ms_events > 0
    assert 0.5 < ms_clock / ms_events < 2.0, (ms_clock / n, ms_events / n)
