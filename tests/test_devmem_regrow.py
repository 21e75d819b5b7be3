"""Buffers of the host runtime that grow on demand (kg_devmem.h, `grow` in kg_runtime.cpp), each taken through one
regrow on one context and one PodBatch object, the results before and after it against the CPU oracle:
kg_eval_diagnose's scratch (64-row floor -> 200 rows), the row list that kg_eval_diagnose, kg_eval_feasible and
kg_eval_offer_slots stage in one buffer (10 -> 200 -> 33 -> 10 rows, call after call), the select's partial rows (300 -> 5,000 nodes and back), the
candidate node-set tables (2 -> 40 sets) and the row-update staging (256-row floor -> 400 rows).

Bar: bit-exact (np.array_equal): counts, keys, status words and node state are integers."""
import functools

import numpy as np
import pytest

import node_sets_ref as ref
import offer_slots_ref
import oracle_lib
from koordinator_amd import abi, engine, nodesets, synth
from test_diagnose import assert_counts, expected
from test_feasible import expected as feasible_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def cluster(n_nodes, n_pods, seed):
    cfg, nodes, pods = synth.small(n_nodes, n_pods, seed=seed, numa=True)
    return cfg.kg_config(), nodes, pods


@pytest.fixture(scope="module")
def batch(ctx):
    """The one PodBatch of the module: every test uploads its own pods into it."""
    b = engine.PodBatch(ctx, cluster(300, 256, 21)[2], capacity=256)
    yield b
    b.close()


def test_diagnose_regrow(ctx, batch):
    kc, nodes, pods = cluster(300, 256, 21)
    want = expected(oracle_lib.eval_verify(kc, nodes, pods).status, True)
    snap = engine.Snapshot(ctx, kc, nodes)
    batch.upload(pods)
    few = np.arange(250, 240, -1, dtype=np.uint32)  # 10 rows: the 64-row floor
    assert_counts(engine.eval_diagnose(snap, batch, rows=few), want[few], "10 rows")
    many = np.arange(200, dtype=np.uint32)[::-1].copy()  # 200 rows: the scratch regrows
    assert_counts(engine.eval_diagnose(snap, batch, rows=many), want[many], "200 rows")
    assert_counts(engine.eval_diagnose(snap, batch, rows=few), want[few], "10 rows again")
    assert want[:200].any() and not np.array_equal(want[few], want[many[:10]])


def test_row_list_is_each_calls_own(ctx, batch):
    """kg_eval_diagnose, kg_eval_feasible and kg_eval_offer_slots stage their row lists in one buffer of the batch:
    each call uploads its own list, so no call may see the list of the call before it. Every list here gives another
    result than the list a stale buffer would hold in its place (asserted on the oracle's side below)."""
    kc, nodes, pods = cluster(300, 256, 21)
    status = oracle_lib.eval_verify(kc, nodes, pods).status
    counts, bits = expected(status, True), feasible_bits(status, 0xFFFFFFFF)
    snap = engine.Snapshot(ctx, kc, nodes)
    batch.upload(pods)
    few = np.arange(250, 240, -1, dtype=np.uint32)  # 10 rows: the 64-row floor
    many = np.arange(200, dtype=np.uint32)[::-1].copy()  # 200 rows: the shared list regrows
    gang = np.concatenate([np.arange(60, 82), np.arange(60, 71)]).astype(np.uint32)  # 33 rows, 11 of them twice
    slots = {name: offer_slots_ref.offer_slots(kc, nodes, pods, rows)
             for name, rows in (("gang", gang), ("gang[:10]", gang[:10]), ("many[:33]", many[:33]))}
    # a call that kept the list before it would be seen: the lists' results differ
    assert not np.array_equal(counts[few], counts[many[:10]]) and not np.array_equal(bits[few], bits[many[:10]])
    assert not np.array_equal(counts[few], counts[gang[:10]])
    for stale in ("gang[:10]", "many[:33]"):
        assert not np.array_equal(slots["gang"][0], slots[stale][0]), stale
        assert not np.array_equal(slots["gang"][1], slots[stale][1]), stale
    assert_counts(engine.eval_diagnose(snap, batch, rows=few), counts[few], "10 rows")
    assert np.array_equal(engine.eval_feasible(snap, batch, rows=many), bits[many])
    got = engine.eval_offer_slots(snap, batch, rows=gang, status=True)
    assert np.array_equal(got[0], slots["gang"][0]) and np.array_equal(got[1], slots["gang"][1])
    assert_counts(engine.eval_diagnose(snap, batch, rows=few), counts[few], "10 rows again")
    assert np.array_equal(engine.eval_feasible(snap, batch, rows=few), bits[few])


def test_partial_rows_regrow(ctx, batch, monkeypatch):
    kc, nodes, pods = cluster(300, 64, 22)
    _, big, _ = cluster(5000, 64, 23)
    small_snap = engine.Snapshot(ctx, kc, nodes)
    big_snap = engine.Snapshot(ctx, kc, big)
    batch.upload(pods)
    want_small, want_big = oracle_lib.select(kc, nodes, pods, 3), oracle_lib.select(kc, big, pods, 3)
    assert want_small.any() and want_big.any()
    assert np.array_equal(engine.eval_select(small_snap, batch, 3), want_small)
    assert np.array_equal(engine.eval_select(big_snap, batch, 3), want_big)
    assert np.array_equal(engine.eval_select(small_snap, batch, 3), want_small)
    # The fused top-3 select of fast lanes inserts by atomics and asks for one partial entry, whatever the node count.
    # The two-launch form of the one-pod-block top-1 select (both switches are read per call) keeps partial rows per
    # chunk of records: 5,000 nodes make more chunks than 300, so this is where the partial rows regrow.
    lanes, fast = batch.select_lanes()
    assert lanes == fast  # fast lanes only: the one-pod-block select takes the batch
    monkeypatch.setenv("KG_SMALL_ALLOW_BIG", "1")
    monkeypatch.setenv("KG_NO_SMALL_FUSED_FINISH", "1")
    for snap, table in ((small_snap, nodes), (big_snap, big), (small_snap, nodes)):
        assert np.array_equal(engine.eval_select(snap, batch, 1), oracle_lib.select(kc, table, pods, 1)), snap.n


def test_node_sets_regrow(ctx, batch):
    kc, nodes, pods = cluster(300, 64, 22)
    n, p = abi.table_len(nodes), abi.table_len(pods)
    ver = oracle_lib.eval_verify(kc, nodes, pods)
    snap = engine.Snapshot(ctx, kc, nodes)
    batch.upload(pods)
    rng = np.random.default_rng(24)
    half = np.arange(n) < n // 2
    two = np.where((np.arange(p) % 2 == 0)[:, None], half[None, :], ~half[None, :])
    forty = (rng.random((40, n)) < 0.5)[np.arange(p) % 40]
    for mask, n_sets in ((two, 2), (forty, 40)):  # the second descriptor regrows both tables
        pod_set, bits = nodesets.from_mask(mask)
        assert len(bits) == n_sets
        batch.set_node_sets(pod_set, bits, n)
        for k in (1, 3):
            got = engine.eval_select(snap, batch, k)
            assert np.array_equal(got, ref.expected_keys(ver.status, ver.total, mask, k)), (n_sets, k)
        got = engine.eval_verify(snap, batch)
        assert np.array_equal(got.status, ref.expected_status(ver.status, mask)), n_sets
        assert np.array_equal(got.total, np.where(mask, ver.total, -1)), n_sets
    assert not np.array_equal(ref.expected_keys(ver.status, ver.total, two, 1), ref.expected_keys(ver.status, ver.total, forty, 1))


def test_staging_regrow(ctx, batch):
    kc, nodes, pods = cluster(600, 64, 25)
    snap = engine.Snapshot(ctx, kc, nodes)
    batch.upload(pods)
    merged = {k: v.copy() for k, v in nodes.items()}
    rng = np.random.default_rng(26)
    for n_rows in (10, 400):  # 400 rows: past the staging's 256-row floor
        rows = np.sort(rng.choice(600, n_rows, replace=False)).astype(np.uint32)
        upd = {k: v.copy() for k, v in abi.take(merged, rows.astype(np.int64)).items()}
        upd["req_cpu"] += rng.integers(1, 500, n_rows)  # the storage class stays: the staged path, no regrouping
        upd["req_mem"] += rng.integers(1, 1 << 20, n_rows)
        upd["num_pods"] += 1
        snap.update_rows(rows, upd)
        for k in upd:
            merged[k][rows] = upd[k]
        state = snap.read_state()
        for k in ("req_cpu", "req_mem", "req_eph", "num_pods", "nz_cpu", "nz_mem"):
            assert np.array_equal(state[k], merged[k]), (n_rows, k)
        got, want = engine.eval_verify(snap, batch), oracle_lib.eval_verify(kc, merged, pods)
        for name in ("status", "score_nrf", "score_la", "score_numa", "total", "numa_zone"):
            assert np.array_equal(getattr(got, name), getattr(want, name)), (n_rows, name)
