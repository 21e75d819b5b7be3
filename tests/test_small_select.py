"""The one-pod-block fused top-1 plain select (k_select_small + k_small_finish, select_small in kg_runtime.cpp): one
select launch over both storage classes with the F_BIG records inline, per-chunk slots instead of atomicMax, and a
finish launch that writes every row's key and status (no memset, no k_big_sel, no k_expand_keys). It serves top-1
launches of at most 256 fast lanes and no integer lane, with or without the pod-row reduction.

Every case compares the whole batch with the oracle and with the same call under KG_NO_SMALL_SELECT=1 (read per call:
the general path), keys and result_status. The cluster is test_pod_dedup.py's: synth.mixed(1000, 300, seed=71), both
storage classes and F_BIG records. Its F_BIG share is above the share up to which select_small takes the path, so the
cases lift that gate with KG_SMALL_ALLOW_BIG=1 (read per call) and also check the gated call."""
import numpy as np
import pytest

import oracle_lib
from koordinator_amd import abi, synth
from test_pod_dedup import N_NODES, cluster, distinct_rows, first_rows, tiled_small, wave_kind


def fast_distinct(n):
    """n pairwise distinct pods, all fast lanes (synth.small's pods, req_eph made unique)."""
    _, _, base = synth.small(300, 300, seed=9)
    pods = abi.take(base, np.arange(n) % 300)
    pods["req_eph"] = (pods["req_eph"] + np.arange(n)).astype(np.int64)
    assert all(wave_kind(pods, j) < 3 for j in range(n)) and distinct_rows(pods) == n
    return pods


def is_big(nodes):
    """Records surely outside the float64 fast path (F_BIG): Restricted nodes and node CPU bind policies."""
    return (nodes["numa_policy"] == abi.KG_NUMA_RESTRICTED) | (nodes["cpu_bind_policy"] != 0)


def is_prime(x):
    return x > 1 and all(x % d for d in range(2, int(x ** 0.5) + 1))


def test_inputs():
    """CPU side of the cases below: the batches are fast lanes only, the sub-clusters are what their names say."""
    kc, nodes, lsr_pods = cluster()
    pods = tiled_small()
    assert all(wave_kind(pods, j) < 3 for j in range(300)) and distinct_rows(pods) < 64
    assert distinct_rows(fast_distinct(257)) == 257
    m, n0, n1 = ragged_count(nodes)
    assert is_prime(n0) and is_prime(n1) and n0 > 64 and n1 > 64 and n0 + n1 == m
    # some pod's winning node is an F_BIG record on the F_BIG-heavy sub-cluster (on the whole cluster none is)
    sub = abi.take(nodes, big_heavy(nodes))
    win = abi.key_node(oracle_lib.select(kc, sub, pods, 1)[:, 0])
    assert is_big(sub)[win[win >= 0]].sum() >= 100
    # pods that fit no node, still inside the fast value domain
    assert not oracle_lib.select(kc, nodes, unfit(pods), 1).any()


def ragged_count(nodes):
    """A node count whose class-0 and class-1 counts are primes above 64: no chunk length divides either."""
    single = nodes["numa_policy"] == abi.KG_NUMA_SINGLE_NODE
    for m in range(N_NODES, 0, -1):
        n1 = int(single[:m].sum())
        if is_prime(n1) and is_prime(m - n1):
            return m, m - n1, n1
    raise AssertionError("no such count")


def big_heavy(nodes):
    return np.flatnonzero(is_big(nodes) | (np.arange(N_NODES) % 10 == 0))


def unfit(pods):
    out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in pods.items()}
    out["req_cpu"] = np.full_like(out["req_cpu"], 10 ** 9)  # a million cores, below 2^44
    out["nz_cpu"] = out["req_cpu"].copy()
    out["flags"] = out["flags"] | np.uint32(abi.KG_POD_HAS_CPU)
    return out


@pytest.fixture(scope="module")
def gpu():
    from koordinator_amd import engine
    kc, nodes, lsr_pods = cluster()
    ctx = engine.Context(0)
    snap = engine.Snapshot(ctx, kc, nodes)
    yield ctx, snap, kc, nodes, lsr_pods
    ctx.close()


def select_both(snap, batch, monkeypatch):
    """(keys, status) of the top-1 select on the default path, after checking that the general path
    (KG_NO_SMALL_SELECT=1) gives the same keys and status."""
    from koordinator_amd import engine
    # the cluster's F_BIG share is above select_small's gate: KG_SMALL_ALLOW_BIG (read per call) lifts it
    monkeypatch.setenv("KG_SMALL_ALLOW_BIG", "1")
    keys = engine.eval_select(snap, batch, 1)
    status = engine.result_status(batch)
    monkeypatch.delenv("KG_SMALL_ALLOW_BIG")
    gated = engine.eval_select(snap, batch, 1)  # whichever path the gate picks
    gated_status = engine.result_status(batch)
    monkeypatch.setenv("KG_NO_SMALL_SELECT", "1")
    keys0 = engine.eval_select(snap, batch, 1)
    status0 = engine.result_status(batch)
    monkeypatch.delenv("KG_NO_SMALL_SELECT")
    bad = np.flatnonzero((keys != keys0).any(axis=1))
    assert not len(bad), ("keys differ from the general path", bad[:8])
    assert np.array_equal(status, status0), ("status differs from the general path", np.flatnonzero(status != status0)[:8])
    assert np.array_equal(gated, keys0) and np.array_equal(gated_status, status0)
    return keys, status


def check(snap, kc, nodes, batch, pods, monkeypatch, lanes):
    """The launch has `lanes` fast lanes and no others; keys equal the oracle's and the general path's on every row."""
    got_lanes, fast = batch.select_lanes()
    assert (got_lanes, fast) == (lanes, lanes)
    keys, status = select_both(snap, batch, monkeypatch)
    want = oracle_lib.select(kc, nodes, pods, 1)
    bad = np.flatnonzero((keys != want).any(axis=1))
    assert not len(bad), ("keys differ from the oracle", bad[:8])
    return keys, status


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [1, 64, 65, 256, 257])
def test_lane_counts(gpu, monkeypatch, lanes):
    """All-distinct batches (no rep list): smallest batch, the wave boundary, the full block; 257 lanes are the general
    path's (more than one pod block)."""
    from koordinator_amd import engine
    ctx, snap, kc, nodes, _ = gpu
    pods = fast_distinct(lanes)
    batch = engine.PodBatch(ctx, pods)
    try:
        keys, _ = check(snap, kc, nodes, batch, pods, monkeypatch, lanes)
        assert (keys != 0).any()
    finally:
        batch.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["tiled_300", "distinct_200"])
def test_dedup(gpu, monkeypatch, shape):
    """300 rows of fewer than 64 distinct ones (the finish serves the duplicates through rep) and 200 all-distinct
    rows (gate off: no rep)."""
    from koordinator_amd import engine
    ctx, snap, kc, nodes, _ = gpu
    pods = tiled_small() if shape == "tiled_300" else fast_distinct(200)
    batch = engine.PodBatch(ctx, pods)
    try:
        keys, status = check(snap, kc, nodes, batch, pods, monkeypatch, distinct_rows(pods))
        first = first_rows(pods)
        assert np.array_equal(keys, keys[first]) and np.array_equal(status, status[first])
        assert (keys != 0).any() and not status.any()
    finally:
        batch.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["class0_only", "class1_only", "eight_nodes", "ragged", "zero_nodes", "big_heavy"])
def test_snapshots(gpu, monkeypatch, case):
    """Snapshots with one storage class, fewer nodes than one chunk, class sizes no chunk length divides, no node at
    all, and mostly F_BIG records (there the winners are F_BIG records: test_inputs)."""
    from koordinator_amd import engine
    ctx, _, kc, nodes, _ = gpu
    single = nodes["numa_policy"] == abi.KG_NUMA_SINGLE_NODE
    pods = tiled_small()
    if case == "eight_nodes":
        from test_wave_kinds import edge_cluster
        cfg8, sub, pods8 = edge_cluster(21, n_nodes=8, n_pods=400)
        kc = cfg8.kg_config()
        pods = abi.take(pods8, np.flatnonzero([wave_kind(pods8, j) < 3 for j in range(400)])[:200])
    else:
        idx = {"class0_only": np.flatnonzero(~single), "class1_only": np.flatnonzero(single),
               "ragged": np.arange(ragged_count(nodes)[0]), "zero_nodes": np.arange(0),
               "big_heavy": big_heavy(nodes)}[case]
        sub = abi.take(nodes, idx)
    snap = engine.Snapshot(ctx, kc, sub)
    batch = engine.PodBatch(ctx, pods)
    try:
        lanes = batch.select_lanes()[0]
        assert lanes <= 256
        keys, status = check(snap, kc, sub, batch, pods, monkeypatch, lanes)
        assert (keys != 0).any() == (case != "zero_nodes")
        if case == "zero_nodes":
            assert not status.any()
    finally:
        batch.close()
        snap.close()


@pytest.mark.gpu
@pytest.mark.parametrize("setting", ["48,36,2", "7,5,1", "64,64,3"])
def test_geometry_settings(gpu, monkeypatch, setting):
    """KG_SMALL_CHUNKS="c0,c1,copies" (read per call): the launch-bound variant without scratch (copies x lanes up to
    512 threads), one copy with short chunks, and class-1 chunks as long as class-0 ones, on the batch with duplicates
    and on the F_BIG-heavy snapshot."""
    from koordinator_amd import engine
    ctx, snap, kc, nodes, _ = gpu
    pods = tiled_small()
    sub = abi.take(nodes, big_heavy(nodes))
    snap2 = engine.Snapshot(ctx, kc, sub)
    batch = engine.PodBatch(ctx, pods)
    monkeypatch.setenv("KG_SMALL_CHUNKS", setting)
    try:
        keys, _ = check(snap, kc, nodes, batch, pods, monkeypatch, distinct_rows(pods))
        assert (keys != 0).any()
        check(snap2, kc, sub, batch, pods, monkeypatch, distinct_rows(pods))
    finally:
        batch.close()
        snap2.close()


@pytest.mark.gpu
def test_path_is_taken(gpu, monkeypatch):
    """The gated default call really runs the two-launch path on a snapshot without F_BIG records (what config 2 is):
    its device time inside the profile bracket is below the general path's. The general path runs two memsets,
    k_select1 per storage class, k_big_sel and k_expand_keys one after the other, the small path two kernels over the
    same records, so a select that fell back to the general path would measure the same as KG_NO_SMALL_SELECT=1
    instead. Keys and status are compared as in every other case; the figures are printed."""
    from koordinator_amd import engine
    ctx, _, kc, nodes, _ = gpu
    sub = abi.take(nodes, np.flatnonzero(~is_big(nodes) & (nodes["numa_policy"] != abi.KG_NUMA_BEST_EFFORT)))
    pods = tiled_small()
    snap = engine.Snapshot(ctx, kc, sub)
    batch = engine.PodBatch(ctx, pods)

    def bracket_ms(n=40):
        for _ in range(5):
            engine.eval_select_async(snap, batch, 1)
        ctx.sync()
        ctx.profile(True)
        ctx.profile_read(reset=True)
        for _ in range(n):
            engine.eval_select_async(snap, batch, 1)
        ctx.sync()
        ms, launches = ctx.profile_read(reset=True)
        ctx.profile(False)
        assert launches == n
        return ms / n

    try:
        check(snap, kc, sub, batch, pods, monkeypatch, distinct_rows(pods))
        small = bracket_ms()
        monkeypatch.setenv("KG_NO_SMALL_SELECT", "1")
        general = bracket_ms()
        monkeypatch.delenv("KG_NO_SMALL_SELECT")
        print(f"bracket ms per select: default {small:.5f}, KG_NO_SMALL_SELECT {general:.5f}")
        assert small < general
    finally:
        batch.close()
        snap.close()


@pytest.mark.gpu
def test_stale_results(gpu, monkeypatch):
    """Nothing is zeroed before a launch, so every row must be rewritten: after a select with feasible pods the same
    batch object takes pods that fit no node, with another duplicate structure, and every key and status is 0; two
    selects in a row agree (the slots are reused)."""
    from koordinator_amd import engine
    ctx, snap, kc, nodes, _ = gpu
    first = tiled_small()
    batch = engine.PodBatch(ctx, first, capacity=300)
    try:
        keys, _ = check(snap, kc, nodes, batch, first, monkeypatch, distinct_rows(first))
        assert (keys != 0).all()
        monkeypatch.setenv("KG_SMALL_ALLOW_BIG", "1")
        for _ in range(2):
            assert np.array_equal(engine.eval_select(snap, batch, 1), keys)
        monkeypatch.delenv("KG_SMALL_ALLOW_BIG")
        second = unfit(abi.take(fast_distinct(120), (np.arange(280) * 7 % 280) // 3))
        batch.upload(second)
        keys, status = check(snap, kc, nodes, batch, second, monkeypatch, distinct_rows(second))
        assert not keys.any() and not status.any()
        batch.upload(first)
        keys, _ = check(snap, kc, nodes, batch, first, monkeypatch, distinct_rows(first))
        assert (keys != 0).all()
    finally:
        batch.close()


@pytest.mark.gpu
@pytest.mark.parametrize("setting", [None, "48,36,2"])
def test_status(gpu, monkeypatch, setting):
    """Nodes holding reservations with NUMA allocations (test_pod_dedup.test_status_on_every_copy): the F_BIG records'
    NodeNUMAResource pairs there are KG_ST_UNSUPPORTED. At k = 1 the flag is equal on every copy of a row and bounded
    by the oracle's flags; keys equal the oracle's and the general path's."""
    from koordinator_amd import engine
    ctx, _, kc, nodes, lsr_pods = gpu
    marked = dict(nodes)
    marked["rsv_numa"] = (np.random.default_rng(5).random(N_NODES) < 0.3).astype(np.uint8)
    fast = np.flatnonzero([wave_kind(lsr_pods, j) < 3 for j in range(300)])[:100]
    pods = abi.take(lsr_pods, np.concatenate([fast, fast[::-1], fast]))  # every row three times
    ref = oracle_lib.eval_verify(kc, marked, pods)
    may = np.bitwise_or.reduce(ref.status & abi.KG_ST_UNSUPPORTED, axis=1)
    assert (may != 0).sum() >= 100
    first = first_rows(pods)
    snap = engine.Snapshot(ctx, kc, marked)
    batch = engine.PodBatch(ctx, pods)
    if setting:  # the launch-bound variant without scratch (test_geometry_settings)
        monkeypatch.setenv("KG_SMALL_CHUNKS", setting)
    try:
        _, status = check(snap, kc, marked, batch, pods, monkeypatch, distinct_rows(pods))
        assert np.array_equal(status, status[first])
        assert not (status & ~may).any() and not (status & ~np.uint32(abi.KG_ST_UNSUPPORTED)).any()
        # as in test_status_on_every_copy: the flag does occur, so the slots' status pair and the finish's decision run
        assert (status[:100] != 0).sum() >= 2
    finally:
        batch.close()
        snap.close()
