"""The finisher's row stores of the one-launch top-1 select (k_select_small, kg_kernels.hip) and the chunk geometry
around them. The finisher reads lane_of as 32-bit words and stores four rows per thread and step as 16-byte vectors
when the host finds lane_of, out and pstat 16-byte aligned (select_local in kg_runtime.cpp), the rows past the last
multiple of four and every row of an unaligned table one by one: row counts around multiples of four and around the
workgroup's 1,024 threads, and a sharded select whose key table starts an odd number of keys into its buffer.

The other cases walk the chunk bounds that a per-chunk prefetch of the records would have to respect (partial last
chunks, one-record and largest chunks, the table's last record, an empty storage class, adjacent F_BIG records, one and
MAX_ZONES zones, records updated between two selects). Such a warm-up was built and measured no faster (DESIGN.md
section 4) and is not in the kernel; the cases stay as checks of the chunk geometry, which this path derives anew.

Every case compares keys and status bit for bit between the default path and the general path (KG_NO_SMALL_SELECT=1,
read per call), and the keys with the oracle's. KG_SMALL_ALLOW_BIG=1 keeps the F_BIG gate out of the way;
KG_SMALL_CHUNKS="c0,c1,copies" sets the geometry. The snapshots are synth.small's 300 nodes unless the case says
otherwise."""
import numpy as np
import pytest

import oracle_lib
from koordinator_amd import abi, synth
from test_pod_dedup import distinct_rows, tiled_small
from test_small_fused import grouped_big, oracle_keys, small_cluster
from test_small_select import fast_distinct, is_big

SMALL_MAX_CHUNK = 64  # kg_kernels.h
LANES = [1, 64, 65, 145, 256]
CHUNKS = ["7,5,2", "7,6,2", "1,1,1", "64,64,1"]
ROWS = [1, 3, 4, 5, 1023, 1025, 1026]


def class_counts(nodes):
    n1 = int((nodes["numa_policy"] == abi.KG_NUMA_SINGLE_NODE).sum())
    return abi.table_len(nodes) - n1, n1


def one_class(nodes, single):
    return abi.take(nodes, np.flatnonzero((nodes["numa_policy"] == abi.KG_NUMA_SINGLE_NODE) == single))


def zoned(nodes):
    """The snapshot with its SingleNUMANode nodes alternating between one zone and MAX_ZONES zones."""
    t = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in nodes.items()}
    single = np.flatnonzero(t["numa_policy"] == abi.KG_NUMA_SINGLE_NODE)
    nz = t["numa_zones"].copy()
    nz[single[0::2]] = 1
    nz[single[1::2]] = abi.KG_MAX_ZONES
    t["numa_zones"] = nz.astype(np.uint32)
    frac = np.random.default_rng(3).random((abi.KG_MAX_ZONES, 2, abi.table_len(t))) * 0.7
    for z in range(abi.KG_MAX_ZONES):
        zc, zm = t["alloc_cpu"] // nz, t["alloc_mem"] // nz
        t[f"zone_cpu{z}"], t[f"zone_mem{z}"] = zc.astype(np.int64), zm.astype(np.int64)
        t[f"zone_cpu_used{z}"] = (zc * frac[z, 0]).astype(np.int64)
        t[f"zone_mem_used{z}"] = (zm * frac[z, 1]).astype(np.int64)
    return t


def filled(kc, nodes, pods):
    """(rows, their new columns, the merged table): the handful of nodes that win most pods, with no cpu or memory
    left, so that other nodes win pods that they won."""
    win = abi.key_node(oracle_keys(("small", 145), kc, nodes, pods)[:, 0])
    ids, counts = np.unique(win[win >= 0], return_counts=True)
    rows = np.sort(ids[np.argsort(-counts)[:5]]).astype(np.uint32)
    upd = abi.take(nodes, rows.astype(np.int64))
    upd["req_cpu"], upd["req_mem"] = upd["alloc_cpu"].copy(), upd["alloc_mem"].copy()
    merged = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in nodes.items()}
    for k in upd:
        if isinstance(merged.get(k), np.ndarray) and len(merged[k]) == abi.table_len(nodes):
            merged[k][rows] = upd[k]
    return rows, upd, merged


def tiled(n):
    """n rows over synth.small(300, 64)'s pods: fewer than 64 lanes."""
    return abi.take(tiled_small(), np.arange(n) % 64)


def tiled_want(kc, nodes, n):
    return oracle_keys("tiled_64", kc, nodes, tiled(64))[np.arange(n) % 64]


def test_inputs():
    """CPU side: the settings give the shapes that the cases below are about."""
    kc, nodes = small_cluster()
    n0, n1 = class_counts(nodes)
    assert (n0, n1) == (235, 65)
    # "7,5,2": the last class-0 chunk is partial, the 65 class-1 records are 13 whole chunks; "7,6,2": the last chunk
    # of both classes is partial; dozens of chunks either way
    assert n0 % 7 and n1 % 5 == 0 and n1 % 6 and -(-n0 // 7) + -(-n1 // 6) > 24
    # "1,1,1": one record per workgroup; "64,64,1": full chunks of SMALL_MAX_CHUNK records in both classes, a partial
    # class-0 one, and the table's last record (class 1 is stored last) alone in the last chunk
    assert n0 // SMALL_MAX_CHUNK == 3 and n0 % SMALL_MAX_CHUNK and n1 // SMALL_MAX_CHUNK == 1 and n1 % SMALL_MAX_CHUNK == 1
    for lanes in LANES:
        assert distinct_rows(fast_distinct(lanes)) == lanes
    assert class_counts(one_class(nodes, False)) == (n0, 0) and class_counts(one_class(nodes, True)) == (0, n1)
    z = zoned(nodes)
    zones = z["numa_zones"][z["numa_policy"] == abi.KG_NUMA_SINGLE_NODE]
    assert (zones == 1).sum() >= 8 and (zones == abi.KG_MAX_ZONES).sum() >= 8 and set(zones.tolist()) == {1, abi.KG_MAX_ZONES}
    big = np.flatnonzero(is_big(grouped_big()[1]))
    assert len(big) == 24 and big[-1] - big[0] == 23
    # freshness: five or more of the pods that the filled nodes won go to another node
    pods = fast_distinct(145)
    rows, _, merged = filled(kc, nodes, pods)
    before = abi.key_node(oracle_keys(("small", 145), kc, nodes, pods)[:, 0])
    after = abi.key_node(oracle_keys("filled", kc, merged, pods)[:, 0])
    moved = np.isin(before, rows)
    changed = (oracle_keys(("small", 145), kc, nodes, pods) != oracle_keys("filled", kc, merged, pods)).any(axis=1)
    assert 2 <= len(rows) <= 5 and moved.sum() >= 5 and changed[moved].sum() >= 5
    assert ((after != before) & (after >= 0))[moved].sum() >= 5
    assert [n % 4 for n in ROWS] == [1, 3, 0, 1, 3, 1, 2] and ROWS[-3] < 1024 < ROWS[-2]
    assert distinct_rows(tiled(5)) == 5 and 32 < distinct_rows(tiled(1026)) < 64


@pytest.fixture(scope="module")
def gpu():
    from koordinator_amd import engine
    kc, nodes = small_cluster()
    ctx = engine.Context(0)
    snap = engine.Snapshot(ctx, kc, nodes)
    yield ctx, snap, kc, nodes
    ctx.close()


def select2(snap, batch, monkeypatch, want):
    """(keys, status) of the default path under the environment the caller has set, after the same call on the general
    path; the two agree, and the keys equal the oracle's (want)."""
    from koordinator_amd import engine
    monkeypatch.setenv("KG_SMALL_ALLOW_BIG", "1")
    monkeypatch.setenv("KG_NO_SMALL_SELECT", "1")
    keys0 = engine.eval_select(snap, batch, 1)
    status0 = engine.result_status(batch)
    monkeypatch.delenv("KG_NO_SMALL_SELECT")
    keys = engine.eval_select(snap, batch, 1)
    status = engine.result_status(batch)
    bad = np.flatnonzero((keys != keys0).any(axis=1))
    assert not len(bad), ("keys differ from the general path", bad[:8], keys[bad[:8], 0], keys0[bad[:8], 0])
    assert np.array_equal(status, status0), ("status differs from the general path", np.flatnonzero(status != status0)[:8])
    bad = np.flatnonzero((keys != want).any(axis=1))
    assert not len(bad), ("keys differ from the oracle", bad[:8])
    return keys, status


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", LANES)
def test_lane_counts(gpu, monkeypatch, lanes):
    """One lane, the wave boundary on both sides, config 2's 145 lanes, the full block: 16, 16, 8, 5 and 4 copies of
    the lanes per workgroup at the default geometry."""
    from koordinator_amd import engine
    ctx, snap, kc, nodes = gpu
    pods = fast_distinct(lanes)
    batch = engine.PodBatch(ctx, pods)
    try:
        assert batch.select_lanes() == (lanes, lanes)
        keys, _ = select2(snap, batch, monkeypatch, oracle_keys(("small", lanes), kc, nodes, pods))
        assert (keys != 0).any()
    finally:
        batch.close()


@pytest.mark.gpu
@pytest.mark.parametrize("chunks", CHUNKS)
def test_chunks(gpu, monkeypatch, chunks):
    """A partial last chunk in class 0 ("7,5,2": the snapshot's 65 class-1 records are whole chunks of 5) and in both
    classes ("7,6,2"); one record per workgroup; the largest chunk, walked by a workgroup of three waves , the last chunk holding the table's last record alone."""
    from koordinator_amd import engine
    ctx, snap, kc, nodes = gpu
    pods = fast_distinct(145)
    batch = engine.PodBatch(ctx, pods)
    monkeypatch.setenv("KG_SMALL_CHUNKS", chunks)
    try:
        keys, _ = select2(snap, batch, monkeypatch, oracle_keys(("small", 145), kc, nodes, pods))
        assert (keys != 0).any()
    finally:
        batch.close()


@pytest.mark.gpu
@pytest.mark.parametrize("single", [False, True])
@pytest.mark.parametrize("chunks", [None, "64,64,1"])
def test_empty_class(gpu, monkeypatch, single, chunks):
    """A snapshot without SingleNUMANode nodes and one of such nodes only: the other class has no chunk."""
    from koordinator_amd import engine
    ctx, _, kc, nodes = gpu
    sub = one_class(nodes, single)
    pods = fast_distinct(145)
    snap = engine.Snapshot(ctx, kc, sub)
    batch = engine.PodBatch(ctx, pods)
    if chunks:
        monkeypatch.setenv("KG_SMALL_CHUNKS", chunks)
    try:
        keys, _ = select2(snap, batch, monkeypatch, oracle_keys(("one_class", single), kc, sub, pods))
        assert (keys != 0).any()
    finally:
        batch.close()
        snap.close()


@pytest.mark.gpu
@pytest.mark.parametrize("chunks", [None, "7,5,2"])
def test_big_records(gpu, monkeypatch, chunks):
    """24 adjacent F_BIG records: the ballot that finds them and the inline integer path behind the fast loops."""
    from koordinator_amd import engine
    ctx = gpu[0]
    kc, sub = grouped_big()
    pods = tiled_small()
    snap = engine.Snapshot(ctx, kc, sub)
    batch = engine.PodBatch(ctx, pods)
    if chunks:
        monkeypatch.setenv("KG_SMALL_CHUNKS", chunks)
    try:
        keys, _ = select2(snap, batch, monkeypatch, oracle_keys("grouped_big", kc, sub, pods))
        assert (keys != 0).any()
    finally:
        batch.close()
        snap.close()


@pytest.mark.gpu
@pytest.mark.parametrize("chunks", [None, "7,5,2"])
def test_zone_counts(gpu, monkeypatch, chunks):
    """SingleNUMANode records with one zone and with MAX_ZONES zones: the zone walk stops after the first
    zone and runs through all of them."""
    from koordinator_amd import engine
    ctx, _, kc, nodes = gpu
    sub = zoned(nodes)
    pods = fast_distinct(145)
    snap = engine.Snapshot(ctx, kc, sub)
    batch = engine.PodBatch(ctx, pods)
    if chunks:
        monkeypatch.setenv("KG_SMALL_CHUNKS", chunks)
    try:
        keys, _ = select2(snap, batch, monkeypatch, oracle_keys("zoned", kc, sub, pods))
        assert (keys != 0).any()
    finally:
        batch.close()
        snap.close()


@pytest.mark.gpu
def test_freshness(gpu, monkeypatch):
    """Select, fill the nodes that won most pods (Snapshot.update_rows), select again with the same batch: the second
    result is the oracle's on the updated table."""
    from koordinator_amd import engine
    ctx, _, kc, nodes = gpu
    pods = fast_distinct(145)
    rows, upd, merged = filled(kc, nodes, pods)
    snap = engine.Snapshot(ctx, kc, nodes)
    batch = engine.PodBatch(ctx, pods)
    try:
        monkeypatch.setenv("KG_SMALL_ALLOW_BIG", "1")
        first = engine.eval_select(snap, batch, 1)
        assert np.array_equal(first, oracle_keys(("small", 145), kc, nodes, pods))
        snap.update_rows(rows, upd)
        want = oracle_keys("filled", kc, merged, pods)
        second = engine.eval_select(snap, batch, 1)
        assert np.array_equal(second, want), np.flatnonzero((second != want).any(axis=1))[:8]
        assert (second != first).any()
        select2(snap, batch, monkeypatch, want)
    finally:
        batch.close()
        snap.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n_rows", ROWS)
def test_row_tail(gpu, monkeypatch, n_rows):
    """Row counts below, at and past a multiple of four, and around the finisher's 1,024 threads, over fewer than 64
    lanes: every row is written (the batch is new: its tables hold no earlier result) and equals the general path."""
    from koordinator_amd import engine
    ctx, snap, kc, nodes = gpu
    pods = tiled(n_rows)
    batch = engine.PodBatch(ctx, pods)
    try:
        assert batch.select_lanes()[0] == distinct_rows(pods) < 64
        monkeypatch.setenv("KG_SMALL_ALLOW_BIG", "1")
        want = tiled_want(kc, nodes, n_rows)
        keys = engine.eval_select(snap, batch, 1)  # the first select of the batch: on the one-launch path
        assert np.array_equal(keys, want), np.flatnonzero((keys != want).any(axis=1))[:8]
        keys, _ = select2(snap, batch, monkeypatch, want)
        assert (keys != 0).any()
    finally:
        batch.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n_rows", [1023, 1026])
def test_unaligned_key_table(gpu, n_rows):
    """A sharded select (one shard) writes its keys n_rows keys into the gather buffer: 8-byte aligned only for the odd
    count, where the finisher must store row by row; 16-byte aligned for the even one."""
    from koordinator_amd import engine
    _, _, kc, nodes = gpu
    pods = tiled(n_rows)
    want = tiled_want(kc, nodes, n_rows)
    sctx = engine.Context(0)
    try:
        sctx.shard_init(engine.shard_unique_id(), 0, 1)
        snap = engine.Snapshot(sctx, kc, nodes)
        batch = engine.PodBatch(sctx, pods)
        got = engine.shard_select(snap, batch, 1)
        again = engine.result_keys(batch, 1)
        status = engine.result_status(batch)
    finally:
        sctx.close()
    assert np.array_equal(got, want) and np.array_equal(again, want)
    assert not status.any()
