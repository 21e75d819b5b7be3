"""The plain select evaluates each distinct pod row once per batch (kg_dedup.h, kg_pods_upload) and k_expand_keys
copies the representative's keys and status to its duplicates. Every case compares the full batch with the oracle on a
synth.mixed cluster of 1,000 nodes: both storage classes (SingleNUMANode nodes are class 1) and F_BIG records
(Restricted / BestEffort nodes, node CPU bind policies), with LSR pods on the integer lanes where a case needs them.

Run as a script (`python tests/test_pod_dedup.py OUT.npy`) it writes the engagement batch's keys for k = 1 and 3: the
KG_SELECT_UNFUSED=1 leg needs a process of its own, the library reads that switch once."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # script mode: the package's tree

import oracle_lib
from koordinator_amd import abi, synth

N_NODES = 1000
BIND = abi.KG_POD_CPU_BIND


def cluster():
    cfg, nodes, lsr_pods = synth.mixed(N_NODES, 300, seed=71)
    return cfg.kg_config(), nodes, lsr_pods


def tiled_small():
    """synth.small(300, 64)'s pods tiled to 300 rows."""
    _, _, base = synth.small(300, 64, seed=7)
    return abi.take(base, np.arange(300) % 64)


ROW = ("req_cpu", "req_mem", "req_eph", "sc_req0", "sc_req1", "nz_cpu", "nz_mem", "la_est0", "la_est1", "flags",
       "numa_policy")


def first_rows(pods):
    """Per row the lowest row with the same plain-path inputs."""
    seen = {}
    return np.array([seen.setdefault(tuple(int(pods[c][j]) for c in ROW), j) for j in range(abi.table_len(pods))])


def distinct_rows(pods):
    return len(set(first_rows(pods).tolist()))


def wave_kind(pods, j):
    """0 prod, 1 koord-batch, 2 general fast lane, 3 integer lane (kg_pods_upload's grouping)."""
    from test_wave_kinds import wave_kind as fast_kind
    if int(pods["flags"][j]) & BIND or int(pods["numa_policy"][j]) != abi.KG_NUMA_NONE:
        return 3
    return fast_kind(pods, j)


def test_cluster_has_both_classes_and_big_records():
    kc, nodes, lsr_pods = cluster()
    pol = nodes["numa_policy"]
    assert abi.table_len(nodes) <= 1500
    assert (pol == abi.KG_NUMA_SINGLE_NODE).sum() > 50 and (pol == abi.KG_NUMA_NONE).sum() > 50  # class 1, class 0
    assert ((pol == abi.KG_NUMA_RESTRICTED) | (pol == abi.KG_NUMA_BEST_EFFORT)).sum() > 50  # F_BIG
    assert (nodes["cpu_bind_policy"] != 0).sum() > 10  # F_BIG
    assert ((lsr_pods["flags"] & BIND) != 0).sum() >= 8
    assert distinct_rows(tiled_small()) < 64


@pytest.fixture(scope="module")
def gpu():
    from koordinator_amd import engine
    kc, nodes, lsr_pods = cluster()
    ctx = engine.Context(0)
    snap = engine.Snapshot(ctx, kc, nodes)
    yield ctx, snap, kc, nodes, lsr_pods
    ctx.close()


def check_oracle(gpu, batch, pods, ks=(1, 3)):
    """Keys of the uploaded batch equal the oracle's on the full batch; returns them by k."""
    from koordinator_amd import engine
    ctx, snap, kc, nodes, _ = gpu
    out = {}
    for k in ks:
        got = engine.eval_select(snap, batch, k)
        want = oracle_lib.select(kc, nodes, pods, k)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert not len(bad), (k, bad[:8])
        out[k] = got
    assert (out[ks[0]][:, 0] != 0).any()
    return out


@pytest.mark.gpu
def test_engagement(gpu, monkeypatch, tmp_path):
    from koordinator_amd import engine
    ctx, snap, kc, nodes, _ = gpu
    pods = tiled_small()
    batch = engine.PodBatch(ctx, pods)
    lanes, fast = batch.select_lanes()
    assert lanes == distinct_rows(pods) < 300 and fast <= lanes
    keys = check_oracle(gpu, batch, pods)
    monkeypatch.setenv("KG_NO_POD_DEDUP", "1")
    assert batch.select_lanes()[0] == 300
    for k in (1, 3):
        assert np.array_equal(engine.eval_select(snap, batch, k), keys[k]), k
    monkeypatch.delenv("KG_NO_POD_DEDUP")
    assert batch.select_lanes()[0] == lanes
    # partials + k_merge over the reduced list, then the expansion: a process of its own
    out = tmp_path / "unfused.npy"
    env = dict(os.environ, KG_SELECT_UNFUSED="1")
    subprocess.check_call([sys.executable, os.path.abspath(__file__), str(out)], env=env, timeout=300)
    unfused = np.load(out)
    assert np.array_equal(unfused[:, :1], keys[1]) and np.array_equal(unfused[:, 1:], keys[3])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["two_rows_130", "identical_257", "one_pod"])
def test_small_shapes(gpu, shape):
    from koordinator_amd import engine
    ctx = gpu[0]
    _, _, base = synth.small(300, 64, seed=7)
    a = 0
    b = next(j for j in range(1, 64) if wave_kind(base, j) == wave_kind(base, a) and distinct_rows(abi.take(base, [a, j])) == 2)
    idx, want_lanes = {"two_rows_130": (np.where(np.arange(130) % 3 == 0, a, b), 2),  # one wave serves 130 rows
                       "identical_257": (np.full(257, b), 1),                          # two pod blocks -> one lane
                       "one_pod": (np.array([a]), 1)}[shape]
    pods = abi.take(base, idx)
    batch = engine.PodBatch(ctx, pods)
    assert batch.select_lanes()[0] == want_lanes
    check_oracle(gpu, batch, pods)


@pytest.mark.gpu
def test_integer_lane_duplicates_only(gpu):
    """The only duplicates are integer-lane pods (KG_POD_CPU_BIND pods and pods with a NUMA policy of their own): the
    pruned k_int_* kernels run on the reduced list; every fast pod is distinct."""
    from koordinator_amd import engine
    ctx, _, _, _, lsr_pods = gpu
    lsr = np.flatnonzero((lsr_pods["flags"] & BIND) != 0)[:6]
    plain = np.flatnonzero((lsr_pods["flags"] & BIND) == 0)[:60]
    # 1 + 5 waves reduce to 1 + 1 (the gate asks for at most half the waves)
    idx = np.concatenate([plain, np.tile(lsr, 50), plain[:6], plain[:6]])
    pods = abi.take(lsr_pods, idx)
    n = len(idx)
    pods["numa_policy"] = pods["numa_policy"].copy()
    pods["numa_policy"][-12:-6] = abi.KG_NUMA_SINGLE_NODE  # pods with their own policy, each twice
    pods["numa_policy"][-6:] = abi.KG_NUMA_SINGLE_NODE
    fast = np.arange(n) < 60
    pods["req_eph"] = np.where(fast, pods["req_eph"] + np.arange(n), pods["req_eph"]).astype(np.int64)
    assert all(wave_kind(pods, j) == 3 for j in range(60, n)) and all(wave_kind(pods, j) < 3 for j in range(60))
    batch = engine.PodBatch(ctx, pods)
    lanes, nfast = batch.select_lanes()
    assert nfast == 60 and lanes == distinct_rows(pods) and lanes - nfast <= 12 < n - 60
    check_oracle(gpu, batch, pods)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["late_first_occurrence", "interleaved_kinds"])
def test_ordering(gpu, case):
    from koordinator_amd import engine
    ctx = gpu[0]
    from test_wave_kinds import edge_cluster
    _, _, base = edge_cluster(21, n_nodes=8, n_pods=400)
    uniq = np.flatnonzero(first_rows(base) == np.arange(400)).tolist()
    by_kind = {k: [j for j in uniq if wave_kind(base, j) == k] for k in (0, 1, 2)}  # distinct rows of each kind
    assert all(len(v) >= 8 for v in by_kind.values())
    if case == "late_first_occurrence":
        # per kind group: a row that occurs once leads the group, the duplicated rows start after it
        idx = []
        for k in (0, 1, 2):
            lead, x, y = by_kind[k][:3]
            idx += [lead] + [x, y] * 40 + [x]
    else:
        # duplicates of three rows of each kind, interleaved over the batch
        rows = [by_kind[k][t] for t in range(3) for k in (0, 1, 2)]
        idx = [rows[t % 9] for t in range(9 * 30)] + [by_kind[2][5], by_kind[0][5]]
    pods = abi.take(base, np.array(idx))
    batch = engine.PodBatch(ctx, pods)
    assert batch.select_lanes()[0] == distinct_rows(pods) < len(idx)
    check_oracle(gpu, batch, pods)


@pytest.mark.gpu
def test_gate_off_when_every_pod_differs(gpu):
    from koordinator_amd import engine
    ctx = gpu[0]
    pods = tiled_small()
    pods["req_eph"] = (pods["req_eph"] + np.arange(300)).astype(np.int64)
    batch = engine.PodBatch(ctx, pods)
    assert batch.select_lanes()[0] == 300
    check_oracle(gpu, batch, pods)


@pytest.mark.gpu
def test_reupload(gpu):
    """One batch object, three uploads: 300 rows with 50 distinct, 120 distinct rows, 300 rows with another duplicate
    structure: nothing of an earlier upload's lists survives."""
    from koordinator_amd import engine
    ctx = gpu[0]
    _, _, base = synth.small(300, 300, seed=9)
    uniq = np.flatnonzero(first_rows(base) == np.arange(300)).tolist()
    first = abi.take(base, np.array(uniq[:50])[np.arange(300) % 50])
    second = abi.take(base, np.arange(120) + 100)
    second["req_eph"] = (second["req_eph"] + np.arange(120)).astype(np.int64)
    third = abi.take(base, np.array(uniq[40:110])[(np.arange(300) * 7 % 300) // 5])
    batch = engine.PodBatch(ctx, first, capacity=300)
    assert batch.select_lanes()[0] == distinct_rows(first) == 50
    check_oracle(gpu, batch, first)
    batch.upload(second)
    assert batch.select_lanes()[0] == 120
    check_oracle(gpu, batch, second)
    batch.upload(third)
    assert batch.select_lanes()[0] == distinct_rows(third) == 60
    check_oracle(gpu, batch, third)


@pytest.mark.gpu
def test_status_on_every_copy(gpu):
    """A pod whose select raises KG_ST_UNSUPPORTED shows the flag on every copy (k_expand_keys copies pstat)."""
    from koordinator_amd import engine
    ctx, _, kc, nodes, lsr_pods = gpu
    # nodes holding reservations with NUMA allocations (test_rsv_numa.py): NodeNUMAResource pairs of LSR pods and of
    # nodes with a NUMA policy there are KG_ST_UNSUPPORTED. The select flags a pod when such a pair could change its
    # keys (k_big_sel and the pruned integer lanes skip pairs that cannot), so the oracle's flags bound the device's.
    marked = dict(nodes)
    marked["rsv_numa"] = (np.random.default_rng(5).random(N_NODES) < 0.3).astype(np.uint8)
    idx = np.concatenate([np.arange(300), np.arange(300)[::-1], np.arange(300)])  # every row at least three times
    pods = abi.take(lsr_pods, idx)
    ref = oracle_lib.eval_verify(kc, marked, pods)
    may = np.bitwise_or.reduce(ref.status & abi.KG_ST_UNSUPPORTED, axis=1)
    first = first_rows(pods)
    snap = engine.Snapshot(ctx, kc, marked)
    batch = engine.PodBatch(ctx, pods)
    assert batch.select_lanes()[0] == distinct_rows(pods) <= 300
    for k in (1, 3):
        got = engine.eval_select(snap, batch, k)
        assert np.array_equal(got, oracle_lib.select(kc, marked, pods, k))
        status = engine.result_status(batch)
        assert np.array_equal(status, status[first])
        assert not (status & ~may).any() and not (status & ~np.uint32(abi.KG_ST_UNSUPPORTED)).any()
        assert (status[:300] != 0).sum() >= 2


@pytest.mark.gpu
def test_sharded_world_1(gpu):
    from koordinator_amd import engine
    _, _, kc, nodes, _ = gpu
    pods = tiled_small()
    want = oracle_lib.select(kc, nodes, pods, 3)
    sctx = engine.Context(0)
    try:
        sctx.shard_init(engine.shard_unique_id(), 0, 1)
        snap = engine.Snapshot(sctx, kc, nodes)
        batch = engine.PodBatch(sctx, pods)
        assert batch.select_lanes()[0] < 300
        got = engine.shard_select(snap, batch, 3)
        again = engine.result_keys(batch, 3)
        status = engine.result_status(batch)
    finally:
        sctx.close()
    assert np.array_equal(got, want) and np.array_equal(again, want)
    assert not status.any()


if __name__ == "__main__":
    from koordinator_amd import engine
    assert os.environ.get("KG_SELECT_UNFUSED") == "1"
    kc_, nodes_, _ = cluster()
    pods_ = tiled_small()
    ctx_ = engine.Context(0)
    try:
        snap_ = engine.Snapshot(ctx_, kc_, nodes_)
        batch_ = engine.PodBatch(ctx_, pods_)
        assert batch_.select_lanes()[0] < 300
        np.save(sys.argv[1], np.concatenate([engine.eval_select(snap_, batch_, 1), engine.eval_select(snap_, batch_, 3)], axis=1))
    finally:
        ctx_.close()
