"""A result of the one-launch top-1 select that is kept per lane (launch_small_select and kg_result_keys /
kg_result_status in kg_runtime.cpp, LaneResult in kg_small.h). A kg_eval_select on the batch's own tables keeps one key
and one status word per lane; the two readers copy those and expand the rows on the host through the row -> lane
table of the upload that the select ran on. Since the form without a finisher became the default, the selects below
run k_select_small's SMALL_ACC form (the accumulators are the result, the reader folds the replicas); the finisher's
SMALL_LANES form, which this file was written for, is compared with it on every select of test_small_acc_results.py
(select_acc, KG_SMALL_FINISHER=1). The batch records which form its last result has, so every case below is
about one of: a row that reads the wrong lane, a lane that was not stored, a form flag that outlives its select, or a
table that is not the select's.

Every select is checked three ways, bit for bit: keys against the oracle's, keys and status against the general path
(KG_NO_SMALL_SELECT=1) and against the row form (KG_SMALL_ROW_RESULTS=1), all read per call. KG_SMALL_ALLOW_BIG=1 keeps
the F_BIG gate out of the way. The snapshots are synth.small's 300 nodes (both storage classes) unless the case says
otherwise. A plain batch on a config-5 snapshot is not among the cases: that select never takes the one-launch path, and
no fixture of the suite builds such a snapshot cheaply."""
import numpy as np
import pytest

import node_sets_ref as ref
import oracle_lib
from koordinator_amd import abi, nodesets
from test_pod_dedup import N_NODES, cluster, distinct_rows, first_rows, tiled_small, wave_kind
from test_small_fused import grouped_big, oracle_keys, small_cluster
from test_small_select import fast_distinct, unfit

KG_INVALID_ARG = 1  # include/koordgpu.h
ROWS = [1, 2, 3, 5, 1023]
ENV = ("KG_NO_SMALL_SELECT", "KG_SMALL_ROW_RESULTS", "KG_NO_POD_DEDUP", "KG_SMALL_REPLICAS", "KG_SMALL_PHASES",
       "KG_PROFILE_BOUND_EVENTS", "KG_NO_SMALL_FUSED_FINISH", "KG_SMALL_CHUNKS")


def tiled(n):
    """n rows over synth.small(300, 64)'s pods: fewer than 64 lanes."""
    return abi.take(tiled_small(), np.arange(n) % 64)


def shuffled37():
    """1,000 rows of 37 distinct pods in a shuffled order: neighbouring rows read different lanes."""
    return abi.take(fast_distinct(37), np.random.default_rng(11).permutation(1000) % 37)


def three_pods(n):
    return abi.take(fast_distinct(3), np.arange(n) % 3)


def test_inputs():
    """CPU side: the batches have the row and lane counts that the cases are about."""
    assert [n % 4 for n in ROWS] == [1, 2, 3, 1, 3]
    assert distinct_rows(tiled(5)) == 5 and 32 < distinct_rows(tiled(1023)) < 64
    pods = shuffled37()
    first = first_rows(pods)
    assert distinct_rows(pods) == 37 and abi.table_len(pods) == 1000
    assert (first[1:] != first[:-1]).sum() > 900
    kc, nodes = small_cluster()
    assert not oracle_lib.select(kc, nodes, unfit(fast_distinct(3)), 1).any()
    # the form-change steps: every step's answer differs from the one before, no pair is KG_ST_UNSUPPORTED
    prev = oracle_keys(("small", "tiled"), kc, nodes, tiled_small())
    for step, (_, _, k, want, unsup) in enumerate(form_steps()):
        assert (want[:, :1] != prev).any() and want.shape == (300, k) and not unsup, step
        prev = want[:, :1]


@pytest.fixture(scope="module")
def gpu():
    from koordinator_amd import engine
    kc, nodes = small_cluster()
    ctx = engine.Context(0)
    snap = engine.Snapshot(ctx, kc, nodes)
    yield ctx, snap, kc, nodes
    ctx.close()


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("KG_SMALL_ALLOW_BIG", "1")


def read(snap, batch, k=1):
    from koordinator_amd import engine
    keys = engine.eval_select(snap, batch, k)
    return keys, engine.result_status(batch)


def select4(snap, batch, monkeypatch, want):
    """(keys, status) of the default form under the caller's environment (a result per lane: SMALL_ACC, the
    accumulators folded by the reader), after the same select on the general path and in the row form (SMALL_ROWS4 /
    SMALL_ROWS): all three agree, and the keys are the oracle's (want)."""
    monkeypatch.setenv("KG_NO_SMALL_SELECT", "1")
    keys0, status0 = read(snap, batch)
    monkeypatch.delenv("KG_NO_SMALL_SELECT")
    monkeypatch.setenv("KG_SMALL_ROW_RESULTS", "1")
    keys1, status1 = read(snap, batch)
    monkeypatch.delenv("KG_SMALL_ROW_RESULTS")
    keys, status = read(snap, batch)
    for name, k, s in (("general path", keys0, status0), ("row form", keys1, status1)):
        bad = np.flatnonzero((keys != k).any(axis=1))
        assert not len(bad), (f"keys differ from the {name}", bad[:8], keys[bad[:8], 0], k[bad[:8], 0])
        assert np.array_equal(status, s), (f"status differs from the {name}", np.flatnonzero(status != s)[:8])
    bad = np.flatnonzero((keys != want).any(axis=1))
    assert not len(bad), ("keys differ from the oracle", bad[:8], keys[bad[:8], 0], want[bad[:8], 0])
    return keys, status


def phase_records(path):
    """The records of a KG_SMALL_PHASES file: per one-launch select [workgroups, 4] clock readings."""
    words = np.fromfile(path, np.uint64)
    out, at = [], 0
    while at < len(words):
        nc = int(words[at])
        out.append(words[at + 1:at + 1 + 4 * nc].reshape(nc, 4))
        at += 1 + 4 * nc
    return out


# ---- 1: row and lane counts --------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n_rows", ROWS)
def test_row_counts(gpu, monkeypatch, n_rows):
    """Every residue of the row count mod 4 (the row form's vector stores end there; the host gather has no such
    border), one row, and 1,023 rows over fewer than 64 lanes."""
    from koordinator_amd import engine
    ctx, snap, kc, nodes = gpu
    pods = tiled(n_rows)
    batch = engine.PodBatch(ctx, pods)
    try:
        want = oracle_keys("tiled_64", kc, nodes, tiled(64))[np.arange(n_rows) % 64]
        keys = engine.eval_select(snap, batch, 1)  # the batch's first select: nothing of an earlier one to fall back on
        assert np.array_equal(keys, want), np.flatnonzero((keys != want).any(axis=1))[:8]
        keys, _ = select4(snap, batch, monkeypatch, want)
        assert (keys != 0).any()
    finally:
        batch.close()


@pytest.mark.gpu
@pytest.mark.parametrize("replicas", ["1", "4"])
def test_shuffled_rows(gpu, monkeypatch, replicas):
    """1,000 shuffled rows of 37 distinct pods, with one replica of the accumulators and with four."""
    from koordinator_amd import engine
    ctx, snap, kc, nodes = gpu
    pods = shuffled37()
    batch = engine.PodBatch(ctx, pods)
    monkeypatch.setenv("KG_SMALL_REPLICAS", replicas)
    try:
        assert batch.select_lanes() == (37, 37)
        keys, status = select4(snap, batch, monkeypatch, oracle_keys("shuffled37", kc, nodes, pods))
        first = first_rows(pods)
        assert (keys != 0).any() and len(np.unique(keys)) > 1
        assert np.array_equal(keys, keys[first]) and np.array_equal(status, status[first])
    finally:
        batch.close()


@pytest.mark.gpu
@pytest.mark.parametrize("replicas", ["1", "4"])
@pytest.mark.parametrize("lanes", [64, 65, 256])
def test_lane_counts(gpu, monkeypatch, lanes, replicas):
    """A full wave of lanes, one lane into the second wave (the tables are padded to 128 entries, 63 of them idle) and
    the full block; every row its own lane (no duplicates: the identity table of the upload)."""
    from koordinator_amd import engine
    ctx, snap, kc, nodes = gpu
    pods = fast_distinct(lanes)
    batch = engine.PodBatch(ctx, pods)
    monkeypatch.setenv("KG_SMALL_REPLICAS", replicas)
    try:
        assert batch.select_lanes() == (lanes, lanes)
        keys, _ = select4(snap, batch, monkeypatch, oracle_keys(("small", lanes), kc, nodes, pods))
        assert (keys != 0).any()
    finally:
        batch.close()


@pytest.mark.gpu
def test_dedup_off(gpu, monkeypatch):
    """KG_NO_POD_DEDUP=1: 256 rows of 64 distinct pods run as 256 lanes through the identity table."""
    from koordinator_amd import engine
    ctx, snap, kc, nodes = gpu
    pods = tiled(256)
    batch = engine.PodBatch(ctx, pods)
    monkeypatch.setenv("KG_NO_POD_DEDUP", "1")
    try:
        want = oracle_keys("tiled_64", kc, nodes, tiled(64))[np.arange(256) % 64]
        keys, _ = select4(snap, batch, monkeypatch, want)
        assert (keys != 0).any()
    finally:
        batch.close()


@pytest.mark.gpu
def test_no_feasible_node(gpu, monkeypatch):
    """Rows of two feasible pods and one that fits no node: its rows read key 0 and status 0, the others their keys."""
    from koordinator_amd import engine
    ctx, snap, kc, nodes = gpu
    three = fast_distinct(3)
    bad = unfit(abi.take(three, np.array([2])))
    mixed = {k: (np.concatenate([v[:2], bad[k]]) if isinstance(v, np.ndarray) else v) for k, v in three.items()}
    pods = abi.take(mixed, np.arange(90) * 7 % 3)
    batch = engine.PodBatch(ctx, pods)
    try:
        want = oracle_keys("one_unfit", kc, nodes, pods)
        lane = np.arange(90) * 7 % 3
        assert not want[lane == 2].any() and want[lane != 2].all()
        keys, status = select4(snap, batch, monkeypatch, want)
        assert not status.any()
    finally:
        batch.close()


@pytest.mark.gpu
def test_unsupported_lanes(gpu, monkeypatch):
    """test_small_fused.test_status's cluster (reservations with NUMA allocations on 1,000 nodes with F_BIG records,
    every row three times): KG_ST_UNSUPPORTED is raised for some lanes, and keys and status agree on every copy."""
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
    try:
        keys, status = select4(snap, batch, monkeypatch, oracle_keys("marked", kc, marked, pods))
        assert np.array_equal(status, status[first]) and np.array_equal(keys, keys[first])
        assert not (status & ~np.uint32(abi.KG_ST_UNSUPPORTED)).any()
        assert 2 <= (status[:100] != 0).sum() < 100
    finally:
        batch.close()
        snap.close()


@pytest.mark.gpu
def test_big_records(gpu, monkeypatch):
    """24 adjacent F_BIG records under KG_SMALL_ALLOW_BIG: their workgroups arrive last and one of them finishes."""
    from koordinator_amd import engine
    ctx = gpu[0]
    kc, sub = grouped_big()
    pods = tiled_small()
    snap = engine.Snapshot(ctx, kc, sub)
    batch = engine.PodBatch(ctx, pods)
    try:
        keys, _ = select4(snap, batch, monkeypatch, oracle_keys("grouped_big", kc, sub, pods))
        assert (keys != 0).any()
    finally:
        batch.close()
        snap.close()


# ---- 2: above the row form's gate --------------------------------------------------------------------------------
@pytest.mark.gpu
def test_above_the_row_gate(gpu, monkeypatch, tmp_path):
    """40,000 rows of three distinct pods: the row form gives the one launch up above 32,768 rows, the lane form takes
    it at any row count. The launch's own phase file (KG_SMALL_PHASES, written by the one-launch form only) has one
    record for the lane-form select, in which exactly one workgroup finished, and none for the row form's."""
    from koordinator_amd import engine
    ctx, snap, kc, nodes = gpu
    n = 40000
    pods = three_pods(n)
    batch = engine.PodBatch(ctx, pods)
    try:
        assert batch.select_lanes() == (3, 3)
        want = oracle_keys("three", kc, nodes, fast_distinct(3))[np.arange(n) % 3]
        keys, status = select4(snap, batch, monkeypatch, want)
        assert (keys != 0).any() and not status.any()
        for form, records in (("lanes", 1), ("rows", 0)):
            path = tmp_path / f"{form}.bin"
            monkeypatch.setenv("KG_SMALL_PHASES", str(path))
            if form == "rows":
                monkeypatch.setenv("KG_SMALL_ROW_RESULTS", "1")
            got, st = read(snap, batch)
            monkeypatch.delenv("KG_SMALL_PHASES")
            assert np.array_equal(got, want) and not st.any(), form
            recs = phase_records(path) if path.exists() else []
            assert len(recs) == records, (form, len(recs))
            for r in recs:
                assert (r[:, 3] != 0).sum() == 1 and (r[:, :3] != 0).all()
    finally:
        batch.close()


# ---- 3: the form changes on one batch ----------------------------------------------------------------------------
def fill_winners(kc, nodes, prev_keys):
    """(rows, their new columns, the merged table): the node that wins most pods gets no cpu or memory left."""
    win = abi.key_node(prev_keys[:, 0])
    ids, counts = np.unique(win[win >= 0], return_counts=True)
    rows = np.array([ids[np.argmax(counts)]], np.uint32)
    upd = abi.take(nodes, rows.astype(np.int64))
    upd["req_cpu"], upd["req_mem"] = upd["alloc_cpu"].copy(), upd["alloc_mem"].copy()
    merged = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in nodes.items()}
    for k in upd:
        if isinstance(merged.get(k), np.ndarray) and len(merged[k]) == abi.table_len(nodes):
            merged[k][rows] = upd[k]
    return rows, upd, merged


def half_sets():
    """Even pods may take even nodes only, odd pods odd nodes: (mask, pod_set, bits)."""
    n = abi.table_len(small_cluster()[1])
    half = np.arange(n) % 2 == 0
    mask = np.where((np.arange(300) % 2 == 0)[:, None], half[None, :], ~half[None, :])
    return (mask,) + tuple(nodesets.from_mask(mask))


_steps = []


def form_steps():
    """The steps of test_form_changes after the first select, computed once: (rows to update, their columns, k, the
    expected keys, whether the oracle marks some pair KG_ST_UNSUPPORTED). Step 0 runs with half_sets, the others
    without."""
    if not _steps:
        kc, table = small_cluster()
        pods = tiled_small()
        mask = half_sets()[0]
        prev = oracle_keys(("small", "tiled"), kc, table, pods)
        for sets, k in ((True, 1), (False, 1), (False, 3), (False, 1)):
            rows, upd, table = fill_winners(kc, table, prev)
            ver = oracle_lib.eval_verify(kc, table, pods)
            want = ref.expected_keys(ver.status, ver.total, mask if sets else None, k)
            want.setflags(write=False)
            _steps.append((rows, upd, k, want, bool((ver.status & abi.KG_ST_UNSUPPORTED).any())))
            prev = want[:, :1]
    return _steps


@pytest.mark.gpu
def test_form_changes(gpu, monkeypatch):
    """One batch in turn: a one-launch select (lanes); candidate node sets (general path, rows); sets cleared (lanes);
    k = 3 (rows); k = 1 again (lanes). Before every step the node that won most pods is filled, so each step's answer
    differs from the one before and a form flag left over from it would serve that. Keys against the oracle's verify
    matrix of the updated table (node_sets_ref.expected_keys), status all zero as the oracle's verify words say."""
    from koordinator_amd import engine
    ctx, _, kc, nodes = gpu
    pods = tiled_small()
    _, pod_set, bits = half_sets()
    snap = engine.Snapshot(ctx, kc, nodes)
    batch = engine.PodBatch(ctx, pods)
    try:
        keys, status = read(snap, batch)
        assert np.array_equal(keys, oracle_keys(("small", "tiled"), kc, nodes, pods)) and not status.any()
        for step, (rows, upd, k, want, _) in enumerate(form_steps()):
            snap.update_rows(rows, upd)
            if step == 0:
                batch.set_node_sets(pod_set, bits, snap.n)
            elif step == 1:
                batch.clear_node_sets()
            keys, status = read(snap, batch, k)
            bad = np.flatnonzero((keys != want).any(axis=1))
            assert not len(bad), (step, "keys differ from the oracle", bad[:8])
            assert not status.any(), step
            assert np.array_equal(engine.result_keys(batch, k), want), step
    finally:
        batch.close()
        snap.close()


# ---- 4: reads ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_reads(gpu, monkeypatch):
    """Status before keys, keys twice, status again: one answer. After a later upload and before the next select both
    reads fail with KG_INVALID_ARG "no selection result" (include/koordgpu.h), whatever the new batch's size; the next
    select serves the new batch."""
    from koordinator_amd import engine
    ctx, snap, kc, nodes = gpu
    pods = shuffled37()
    want = oracle_keys("shuffled37", kc, nodes, pods)
    batch = engine.PodBatch(ctx, pods, capacity=2000)
    try:
        engine.eval_select_async(snap, batch, 1)
        status = engine.result_status(batch)
        keys = engine.result_keys(batch, 1)
        assert np.array_equal(keys, want) and not status.any()
        assert np.array_equal(engine.result_keys(batch, 1), want)
        assert np.array_equal(engine.result_status(batch), status)
        for later in (tiled(2000), tiled(5)):
            batch.upload(later)
            for call in (lambda: engine.result_keys(batch, 1), lambda: engine.result_status(batch)):
                with pytest.raises(engine.EngineError, match="no selection result") as e:
                    call()
                assert e.value.status == KG_INVALID_ARG
            m = abi.table_len(later)
            keys, status = read(snap, batch)
            assert np.array_equal(keys, oracle_keys("tiled_64", kc, nodes, tiled(64))[np.arange(m) % 64])
            assert not status.any()
    finally:
        batch.close()


# ---- 5: profiling ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("bound", [False, True])
def test_profiling(gpu, monkeypatch, bound):
    """Profiling on, with the device-clock bracket and with the bound event pair: keys and status are those of
    profiling off, and kg_profile_read counts one launch per select."""
    from koordinator_amd import engine
    ctx, snap, kc, nodes = gpu
    pods = shuffled37()
    batch = engine.PodBatch(ctx, pods)
    try:
        keys_off, status_off = select4(snap, batch, monkeypatch, oracle_keys("shuffled37", kc, nodes, pods))
        if bound:
            monkeypatch.setenv("KG_PROFILE_BOUND_EVENTS", "1")
        ctx.profile(True)
        try:
            ctx.profile_read(reset=True)
            for _ in range(3):
                keys, status = read(snap, batch)
                assert np.array_equal(keys, keys_off) and np.array_equal(status, status_off)
            ms, launches = ctx.profile_read(reset=True)
        finally:
            ctx.profile(False)
        assert launches == 3 and ms > 0
    finally:
        batch.close()
