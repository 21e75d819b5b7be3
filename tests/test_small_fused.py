"""The one-launch form of the one-pod-block top-1 select (k_select_small with small_replicas > 0, select_small /
ensure_sacc in kg_runtime.cpp): the workgroups fold their results into replicated per-lane accumulators by atomic
maxima, take a ticket, and the workgroup that arrives last reads and resets the accumulators and writes every row's key
and status. The accumulators and the ticket are zero between launches and no host call zeroes them in a steady-state
step, so a word left dirty by one launch shows in the next as a wrong key or as a finish that never runs (the rows then
keep what the reference calls below wrote into them: results of another path, or of other pods).

Every case compares keys and status, bit for bit, with three references: the oracle (keys), the general path
(KG_NO_SMALL_SELECT=1) and the two-launch form (KG_NO_SMALL_FUSED_FINISH=1), all read per call. The snapshots are
synth.small's 300 nodes unless the case says otherwise; KG_SMALL_ALLOW_BIG=1 keeps the F_BIG gate out of the way and
KG_SMALL_CHUNKS / KG_SMALL_REPLICAS (measurement aids, read per call) set the chunk and replica counts: on 300 nodes
"8,8,1" and "7,5,2" give dozens of workgroups."""
import numpy as np
import pytest

import oracle_lib
from koordinator_amd import abi, synth
from test_pod_dedup import N_NODES, cluster, distinct_rows, first_rows, tiled_small, wave_kind
from test_small_select import fast_distinct, is_big, unfit

CHUNKS = ["8,8,1", "7,5,2"]
# one replica for all; 3 and 5 (the settings give 39 and 47 chunks: 5 divides neither, 3 only the first); more than chunks
REPLICAS = ["1", "3", "5", "4000"]


def small_cluster():
    cfg, nodes, _ = synth.small(300, 64, seed=7)
    return cfg.kg_config(), nodes


_want = {}


def oracle_keys(tag, kc, nodes, pods):
    """The oracle's top-1 keys, computed once per (snapshot, batch) tag."""
    if tag not in _want:
        _want[tag] = oracle_lib.select(kc, nodes, pods, 1)
        _want[tag].setflags(write=False)
    return _want[tag]


def n_chunks(nodes, c0, c1):
    single = nodes["numa_policy"] == abi.KG_NUMA_SINGLE_NODE
    n1 = int(single.sum())
    n0 = abi.table_len(nodes) - n1
    return -(-n0 // c0) + -(-n1 // c1)


def test_inputs():
    """CPU side: the chunk settings give dozens of workgroups on the 300 nodes, 5 divides neither count, 3 not the
    second, and 4000 is above both; the batches are fast lanes only; the grouped snapshot holds few F_BIG records, next
    to each other."""
    kc, nodes = small_cluster()
    counts = [n_chunks(nodes, 8, 8), n_chunks(nodes, 7, 5)]
    assert all(24 <= c < 4000 and c % 5 for c in counts) and counts[1] % 3, counts
    for lanes in (1, 64, 65, 145, 256):
        assert distinct_rows(fast_distinct(lanes)) == lanes
    assert distinct_rows(tiled_small()) < 64
    sub = grouped_big()[1]
    big = np.flatnonzero(is_big(sub))
    assert 8 <= len(big) <= 32 and big[-1] - big[0] == len(big) - 1
    assert not oracle_lib.select(kc, nodes, unfit(fast_distinct(40)), 1).any()


def grouped_big():
    """300 of the mixed cluster's nodes: 24 F_BIG ones side by side in the middle of nodes that are not."""
    kc, nodes, _ = cluster()
    big = is_big(nodes)
    rest, bigs = np.flatnonzero(~big), np.flatnonzero(big)
    return kc, abi.take(nodes, np.concatenate([rest[:138], bigs[:24], rest[138:276]]))


@pytest.fixture(scope="module")
def gpu():
    from koordinator_amd import engine
    kc, nodes = small_cluster()
    ctx = engine.Context(0)
    snap = engine.Snapshot(ctx, kc, nodes)
    yield ctx, snap, kc, nodes
    ctx.close()


def select3(snap, batch, monkeypatch, want):
    """(keys, status) of the one-launch select under the environment the caller has set, after the same call on the
    two-launch form and on the general path; all three agree, and the keys equal the oracle's (want)."""
    from koordinator_amd import engine
    monkeypatch.setenv("KG_SMALL_ALLOW_BIG", "1")
    monkeypatch.setenv("KG_NO_SMALL_SELECT", "1")
    keys0 = engine.eval_select(snap, batch, 1)
    status0 = engine.result_status(batch)
    monkeypatch.delenv("KG_NO_SMALL_SELECT")
    monkeypatch.setenv("KG_NO_SMALL_FUSED_FINISH", "1")
    keys2 = engine.eval_select(snap, batch, 1)
    status2 = engine.result_status(batch)
    monkeypatch.delenv("KG_NO_SMALL_FUSED_FINISH")
    keys = engine.eval_select(snap, batch, 1)
    status = engine.result_status(batch)
    for name, k, s in (("general path", keys0, status0), ("two-launch form", keys2, status2)):
        bad = np.flatnonzero((keys != k).any(axis=1))
        assert not len(bad), (f"keys differ from the {name}", bad[:8], keys[bad[:8], 0], k[bad[:8], 0])
        assert np.array_equal(status, s), (f"status differs from the {name}", np.flatnonzero(status != s)[:8])
    bad = np.flatnonzero((keys != want).any(axis=1))
    assert not len(bad), ("keys differ from the oracle", bad[:8])
    return keys, status


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [1, 64, 65, 145, 256, "tiled"])
def test_lane_counts(gpu, monkeypatch, lanes):
    """One lane, the wave boundary on both sides, config 2's 145 lanes (three waves, the last partly idle), the full
    block; and 300 rows of fewer than 64 distinct ones, where lane_of maps many rows to one lane. Default geometry and
    replica rule."""
    from koordinator_amd import engine
    ctx, snap, kc, nodes = gpu
    pods = tiled_small() if lanes == "tiled" else fast_distinct(lanes)
    batch = engine.PodBatch(ctx, pods)
    try:
        n = distinct_rows(pods)
        assert batch.select_lanes() == (n, n)
        keys, status = select3(snap, batch, monkeypatch, oracle_keys(("small", lanes), kc, nodes, pods))
        assert (keys != 0).any()
        first = first_rows(pods)
        assert np.array_equal(keys, keys[first]) and np.array_equal(status, status[first])
    finally:
        batch.close()


@pytest.mark.gpu
@pytest.mark.parametrize("replicas", REPLICAS)
@pytest.mark.parametrize("chunks", CHUNKS)
@pytest.mark.parametrize("lanes", [145, "tiled"])
def test_chunks_and_replicas(gpu, monkeypatch, lanes, chunks, replicas):
    """Dozens of workgroups folding into one replica, into three and five (the chunk count is no multiple) and into
    one each (more replicas than chunks), with one and with two copies of the lanes per workgroup."""
    from koordinator_amd import engine
    ctx, snap, kc, nodes = gpu
    pods = tiled_small() if lanes == "tiled" else fast_distinct(lanes)
    batch = engine.PodBatch(ctx, pods)
    monkeypatch.setenv("KG_SMALL_CHUNKS", chunks)
    monkeypatch.setenv("KG_SMALL_REPLICAS", replicas)
    try:
        keys, _ = select3(snap, batch, monkeypatch, oracle_keys(("small", lanes), kc, nodes, pods))
        assert (keys != 0).any()
    finally:
        batch.close()


@pytest.mark.gpu
def test_leftover_state(gpu, monkeypatch):
    """One batch object through the states that a dirty accumulator or ticket word would spoil: three calls in a row;
    then fewer lanes whose pods fit no node (every key 0: an accumulator that kept a key of the calls before shows);
    then other chunk and replica counts from call to call (the arrays are laid out anew over the same zeroed words, and
    the ticket must count to another total); then the first pods again."""
    from koordinator_amd import engine
    ctx, snap, kc, nodes = gpu
    first = fast_distinct(145)
    batch = engine.PodBatch(ctx, first, capacity=300)
    try:
        want = oracle_keys(("small", 145), kc, nodes, first)
        keys, _ = select3(snap, batch, monkeypatch, want)
        monkeypatch.setenv("KG_SMALL_ALLOW_BIG", "1")
        for _ in range(3):
            assert np.array_equal(engine.eval_select(snap, batch, 1), keys)
        second = unfit(abi.take(fast_distinct(40), (np.arange(120) * 7 % 120) // 3))
        batch.upload(second)
        assert batch.select_lanes() == (40, 40)
        for _ in range(2):
            assert not engine.eval_select(snap, batch, 1).any() and not engine.result_status(batch).any()
        keys2, status2 = select3(snap, batch, monkeypatch, np.zeros((120, 1), np.uint64))
        assert not keys2.any() and not status2.any()
        batch.upload(first)
        for chunks, replicas in (("8,8,1", "3"), ("7,5,2", "4000"), ("64,64,5", "1"), ("8,8,1", "2")):
            monkeypatch.setenv("KG_SMALL_CHUNKS", chunks)
            monkeypatch.setenv("KG_SMALL_REPLICAS", replicas)
            assert np.array_equal(engine.eval_select(snap, batch, 1), keys), (chunks, replicas)
        monkeypatch.delenv("KG_SMALL_CHUNKS")
        monkeypatch.delenv("KG_SMALL_REPLICAS")
        select3(snap, batch, monkeypatch, want)
    finally:
        batch.close()


@pytest.mark.gpu
@pytest.mark.parametrize("replicas", ["1", "3"])
def test_uneven_arrival(gpu, monkeypatch, replicas):
    """The F_BIG records of the snapshot sit in a few chunks: those workgroups run the integer path inline and arrive
    long after the others, so the finisher is not the workgroup that was started last."""
    from koordinator_amd import engine
    ctx = gpu[0]
    kc, sub = grouped_big()
    pods = tiled_small()
    snap = engine.Snapshot(ctx, kc, sub)
    batch = engine.PodBatch(ctx, pods)
    monkeypatch.setenv("KG_SMALL_CHUNKS", "8,8,1")
    monkeypatch.setenv("KG_SMALL_REPLICAS", replicas)
    try:
        want = oracle_keys("grouped_big", kc, sub, pods)
        keys, _ = select3(snap, batch, monkeypatch, want)
        assert (keys != 0).any()
        monkeypatch.setenv("KG_SMALL_ALLOW_BIG", "1")
        for _ in range(3):
            assert np.array_equal(engine.eval_select(snap, batch, 1), keys)
    finally:
        batch.close()
        snap.close()


@pytest.mark.gpu
@pytest.mark.parametrize("setting", [None, ("8,8,1", "3")])
def test_status(gpu, monkeypatch, setting):
    """test_small_select.test_status's KG_ST_UNSUPPORTED case (nodes holding reservations with NUMA allocations, every
    row three times) on the one-launch form: the unsupported bounds and the fast keys' high words go through the
    accumulators, the finisher decides the flag."""
    from koordinator_amd import engine
    ctx = gpu[0]
    kc, nodes, lsr_pods = cluster()
    marked = dict(nodes)
    marked["rsv_numa"] = (np.random.default_rng(5).random(N_NODES) < 0.3).astype(np.uint8)
    fast = np.flatnonzero([wave_kind(lsr_pods, j) < 3 for j in range(300)])[:100]
    pods = abi.take(lsr_pods, np.concatenate([fast, fast[::-1], fast]))
    first = first_rows(pods)
    snap = engine.Snapshot(ctx, kc, marked)
    batch = engine.PodBatch(ctx, pods)
    if setting:
        monkeypatch.setenv("KG_SMALL_CHUNKS", setting[0])
        monkeypatch.setenv("KG_SMALL_REPLICAS", setting[1])
    try:
        _, status = select3(snap, batch, monkeypatch, oracle_keys("marked", kc, marked, pods))
        assert np.array_equal(status, status[first])
        assert not (status & ~np.uint32(abi.KG_ST_UNSUPPORTED)).any()
        assert (status[:100] != 0).sum() >= 2
    finally:
        batch.close()
        snap.close()


@pytest.mark.gpu
def test_zero_rows_and_single_chunk(gpu, monkeypatch):
    """A batch without rows launches nothing and leaves the state alone; a snapshot of five nodes of one storage class
    is a single chunk, whose workgroup is first and last to arrive, with one replica and with more."""
    from koordinator_amd import engine
    ctx, snap, kc, nodes = gpu
    pods = fast_distinct(145)
    empty = engine.PodBatch(ctx, abi.take(pods, np.arange(0)), capacity=8)
    single = nodes["numa_policy"] == abi.KG_NUMA_SINGLE_NODE
    sub = abi.take(nodes, np.flatnonzero(~single)[:5])
    snap1 = engine.Snapshot(ctx, kc, sub)
    batch = engine.PodBatch(ctx, pods)
    try:
        monkeypatch.setenv("KG_SMALL_ALLOW_BIG", "1")
        assert engine.eval_select(snap, empty, 1).shape[0] == 0
        monkeypatch.delenv("KG_SMALL_ALLOW_BIG")
        want = oracle_keys("five_nodes", kc, sub, pods)
        for replicas in ("1", "8"):
            monkeypatch.setenv("KG_SMALL_REPLICAS", replicas)
            select3(snap1, batch, monkeypatch, want)
            select3(snap1, batch, monkeypatch, want)
    finally:
        empty.close()
        batch.close()
        snap1.close()
