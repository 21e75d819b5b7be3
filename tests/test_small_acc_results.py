"""The form of the one-launch top-1 select that has no finisher: the accumulators are the result (k_select_small with
SMALL_ACC, kg_kernels.hip; launch_small_select, ensure_acc and fetch_lanes in kg_runtime.cpp, AccParity and fold_acc in
kg_small.h).
Slice 0 of every workgroup folds into one of two parities of the batch's result accumulators and leaves; nothing reads
them back on the device. kg_result_keys / kg_result_status copy the launch's parity, fold the replicas, apply the status
rule and gather the rows on the host. Launch N zeroes what launch N - 1 left in the other parity, so the cases below are
about: an accumulator word that was not zeroed (a key of an earlier, better answer survives: maxima only grow), a dirty
extent that does not follow the replica or lane count, a parity or a form flag that outlives its select, a status word
folded wrongly, and a profile slot that is missing or counted twice.

Every select is checked three ways, bit for bit: keys against the oracle's, keys and status against the general path
(KG_NO_SMALL_SELECT=1) and against the finisher form (KG_SMALL_FINISHER=1: the lane form), all read per call.
KG_SMALL_ALLOW_BIG=1 keeps the F_BIG gate out of the way. The snapshots are synth.small's 300 nodes unless the case says
otherwise."""
import time

import numpy as np
import pytest

import node_sets_ref as ref
import oracle_lib
from koordinator_amd import abi
from test_pod_dedup import N_NODES, cluster, distinct_rows, first_rows, tiled_small, wave_kind
from test_small_fused import grouped_big, n_chunks, oracle_keys, small_cluster
from test_small_lane_results import fill_winners, half_sets, phase_records, shuffled37, three_pods, tiled
from test_small_select import fast_distinct, unfit

KG_INVALID_ARG = 1  # include/koordgpu.h
CUS = 256           # compute units of an MI355X
PROF_SLOTS = 256    # kg_ctx::PROF_SLOTS, kg_runtime.cpp
STALE_STEPS = 6
# test_device_clock_bracket.test_zero_state's sequence: chunk and replica counts change from call to call
LAYOUTS = ((None, None), ("8,8,1", "3"), ("7,5,2", "4000"), ("64,64,5", "1"), ("8,8,1", "2"), (None, None))
ENV = ("KG_NO_SMALL_SELECT", "KG_SMALL_ROW_RESULTS", "KG_SMALL_FINISHER", "KG_NO_POD_DEDUP", "KG_SMALL_REPLICAS",
       "KG_SMALL_PHASES", "KG_PROFILE_BOUND_EVENTS", "KG_NO_SMALL_FUSED_FINISH", "KG_SMALL_CHUNKS")


def one_class_five(nodes):
    """Five records of storage class 0 (no SingleNUMANode policy): one chunk, one workgroup, at any geometry."""
    return abi.take(nodes, np.flatnonzero(nodes["numa_policy"] != abi.KG_NUMA_SINGLE_NODE)[:5])


def one_unfit():
    """90 rows over two feasible pods and one that fits no node; (pods, the lane of every row)."""
    three = fast_distinct(3)
    bad = unfit(abi.take(three, np.array([2])))
    mixed = {k: (np.concatenate([v[:2], bad[k]]) if isinstance(v, np.ndarray) else v) for k, v in three.items()}
    lane = np.arange(90) * 7 % 3
    return abi.take(mixed, lane), lane


_stale = []


def stale_steps():
    """The stale-state sequence, computed once: step 0 is the untouched table; before every later step the node that
    won most pods is filled. Per step (rows to update, their columns, the oracle's keys of the updated table)."""
    if not _stale:
        kc, table = small_cluster()
        pods = tiled_small()
        prev = oracle_keys(("small", "tiled"), kc, table, pods)
        _stale.append((None, None, prev))
        for _ in range(STALE_STEPS):
            rows, upd, table = fill_winners(kc, table, prev)
            want = oracle_lib.select(kc, table, pods, 1)
            want.setflags(write=False)
            _stale.append((rows, upd, want))
            prev = want
    return _stale


FORMS = ("acc", "rows", "acc", "two", "acc", "k3", "acc", "sets", "acc")
_forms = []


def form_steps():
    """The form-change sequence, computed once: per step of FORMS (rows to update or None, their columns, k, the
    expected keys). The winner is filled before every step but the first; "sets" runs under half_sets."""
    if not _forms:
        kc, table = small_cluster()
        pods = tiled_small()
        mask = half_sets()[0]
        prev = oracle_keys(("small", "tiled"), kc, table, pods)
        _forms.append((None, None, 1, prev))
        for form in FORMS[1:]:
            k = 3 if form == "k3" else 1
            rows, upd, table = fill_winners(kc, table, prev)
            ver = oracle_lib.eval_verify(kc, table, pods)
            assert not (ver.status & abi.KG_ST_UNSUPPORTED).any()
            want = ref.expected_keys(ver.status, ver.total, mask if form == "sets" else None, k)
            want.setflags(write=False)
            _forms.append((rows, upd, k, want))
            prev = want[:, :1]
    return _forms


def test_inputs():
    """CPU side. In the stale-state sequence some row's expected key at every step is strictly below its key of one
    step earlier and of two steps earlier (the launch that used the same parity): an accumulator word that kept either
    would show as a key too high. Every form-change step differs from the step before. The batches have the lane and
    row counts their cases claim; one record per workgroup gives more workgroups than compute units."""
    steps = stale_steps()
    assert len(steps) >= 6  # the first select and at least five more
    for i in range(1, len(steps)):
        assert (steps[i][2] < steps[i - 1][2]).any(), i
        if i >= 2:
            assert (steps[i][2] < steps[i - 2][2]).any(), i
    forms = form_steps()
    assert len(forms) == len(FORMS)
    for i in range(1, len(forms)):
        assert (forms[i][3][:, :1] != forms[i - 1][3][:, :1]).any(), i
    kc, nodes = small_cluster()
    assert abi.table_len(nodes) == 300 > CUS
    assert distinct_rows(tiled_small()) < 64 and abi.table_len(tiled_small()) == 300
    for lanes in (3, 64, 65, 256):
        assert distinct_rows(fast_distinct(lanes)) == lanes
    assert distinct_rows(three_pods(40000)) == 3 and abi.table_len(three_pods(40000)) == 40000
    assert distinct_rows(shuffled37()) == 37
    five = one_class_five(nodes)
    assert abi.table_len(five) == 5 and not (five["numa_policy"] == abi.KG_NUMA_SINGLE_NODE).any()
    pods, lane = one_unfit()
    want = oracle_keys("one_unfit", kc, nodes, pods)
    assert not want[lane == 2].any() and want[lane != 2].all()
    # "7,5,2" with 4000 replicas: more replicas than chunks
    assert n_chunks(nodes, 7, 5) < 4000


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


def select_acc(snap, batch, monkeypatch, want):
    """(keys, status) of the default form (the accumulators are the result) under the caller's environment, after the
    same select on the general path and in the finisher form: all three agree, and the keys are the oracle's (want)."""
    monkeypatch.setenv("KG_NO_SMALL_SELECT", "1")
    keys0, status0 = read(snap, batch)
    monkeypatch.delenv("KG_NO_SMALL_SELECT")
    monkeypatch.setenv("KG_SMALL_FINISHER", "1")
    keys1, status1 = read(snap, batch)
    monkeypatch.delenv("KG_SMALL_FINISHER")
    keys, status = read(snap, batch)
    for name, k, s in (("general path", keys0, status0), ("finisher form", keys1, status1)):
        bad = np.flatnonzero((keys != k).any(axis=1))
        assert not len(bad), (f"keys differ from the {name}", bad[:8], keys[bad[:8], 0], k[bad[:8], 0])
        assert np.array_equal(status, s), (f"status differs from the {name}", np.flatnonzero(status != s)[:8])
    bad = np.flatnonzero((keys != want).any(axis=1))
    assert not len(bad), ("keys differ from the oracle", bad[:8], keys[bad[:8], 0], want[bad[:8], 0])
    return keys, status


# ---- 1: stale state ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("replicas", ["1", None])
def test_stale_state(gpu, monkeypatch, replicas):
    """One batch, one snapshot, seven selects of this form in a row and nothing else on the batch in between: keys fall
    from step to step, so a word of either parity that was not zeroed gives a key too high. The references of each
    step run on a second batch."""
    from koordinator_amd import engine
    ctx, _, kc, nodes = gpu
    pods = tiled_small()
    snap = engine.Snapshot(ctx, kc, nodes)
    batch = engine.PodBatch(ctx, pods)
    other = engine.PodBatch(ctx, pods)
    if replicas:
        monkeypatch.setenv("KG_SMALL_REPLICAS", replicas)
    try:
        for step, (rows, upd, want) in enumerate(stale_steps()):
            if rows is not None:
                snap.update_rows(rows, upd)
            keys, status = read(snap, batch)
            bad = np.flatnonzero((keys != want).any(axis=1))
            assert not len(bad), (step, "keys differ from the oracle", bad[:8], keys[bad[:8], 0], want[bad[:8], 0])
            keys2, status2 = select_acc(snap, other, monkeypatch, want)
            assert np.array_equal(keys, keys2) and np.array_equal(status, status2), step
    finally:
        other.close()
        batch.close()
        snap.close()


# ---- 2: layouts that change under the parities -------------------------------------------------------------------
@pytest.mark.gpu
def test_layouts(gpu, monkeypatch):
    """Chunk and replica counts change from call to call, more replicas than chunks among them: the dirty extent of a
    parity is its own launch's, not the next one's."""
    from koordinator_amd import engine
    ctx, snap, kc, nodes = gpu
    pods = tiled_small()
    want = oracle_keys(("small", "tiled"), kc, nodes, pods)
    batch = engine.PodBatch(ctx, pods)
    try:
        for chunks, replicas in LAYOUTS:
            for name, value in (("KG_SMALL_CHUNKS", chunks), ("KG_SMALL_REPLICAS", replicas)):
                if value:
                    monkeypatch.setenv(name, value)
                else:
                    monkeypatch.delenv(name, raising=False)
            for _ in range(2):
                keys, status = read(snap, batch)
                assert np.array_equal(keys, want) and not status.any(), (chunks, replicas)
            select_acc(snap, batch, monkeypatch, want)
    finally:
        batch.close()


@pytest.mark.gpu
def test_shrinking_lane_counts(gpu, monkeypatch):
    """One batch object: 256 distinct lanes, then 65, then 3, each followed by two selects. The lanes beyond the new
    count were dirty in both parities."""
    from koordinator_amd import engine
    ctx, snap, kc, nodes = gpu
    batch = engine.PodBatch(ctx, fast_distinct(256), capacity=256)
    try:
        for lanes in (256, 65, 3):
            pods = fast_distinct(lanes)
            if lanes != 256:
                batch.upload(pods)
            assert batch.select_lanes() == (lanes, lanes)
            want = oracle_keys(("small", lanes), kc, nodes, pods)
            for _ in range(2):
                keys, _ = read(snap, batch)
                assert np.array_equal(keys, want), lanes
            keys, _ = select_acc(snap, batch, monkeypatch, want)
            assert (keys != 0).any()
    finally:
        batch.close()


# ---- 3: the form changes on one batch ----------------------------------------------------------------------------
@pytest.mark.gpu
def test_form_changes(gpu, monkeypatch):
    """FORMS on one batch, the winner filled before each step: this form, the row form, the two launches, k = 3 on the
    general path and candidate node sets in between. The finisher forms keep their own accumulators and this form its
    parities across them; no form flag outlives its select."""
    from koordinator_amd import engine
    ctx, _, kc, nodes = gpu
    pods = tiled_small()
    _, pod_set, bits = half_sets()
    env = {"rows": "KG_SMALL_ROW_RESULTS", "two": "KG_NO_SMALL_FUSED_FINISH"}
    snap = engine.Snapshot(ctx, kc, nodes)
    batch = engine.PodBatch(ctx, pods)
    try:
        for step, (form, (rows, upd, k, want)) in enumerate(zip(FORMS, form_steps())):
            if rows is not None:
                snap.update_rows(rows, upd)
            if form == "sets":
                batch.set_node_sets(pod_set, bits, snap.n)
            if form in env:
                monkeypatch.setenv(env[form], "1")
            if form == "acc":
                keys, status = select_acc(snap, batch, monkeypatch, want)
            else:
                keys, status = read(snap, batch, k)
            if form in env:
                monkeypatch.delenv(env[form])
            bad = np.flatnonzero((keys != want).any(axis=1))
            assert not len(bad), (step, form, "keys differ from the oracle", bad[:8])
            assert not status.any(), (step, form)
            assert np.array_equal(engine.result_keys(batch, k), want), (step, form)
            if form == "sets":
                batch.clear_node_sets()
    finally:
        batch.close()
        snap.close()


# ---- 4: status ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("replicas", ["1", "4"])
def test_unsupported_lanes(gpu, monkeypatch, replicas):
    """test_small_lane_results.test_unsupported_lanes' cluster (reservations with NUMA allocations on 1,000 nodes with
    F_BIG records, every row three times): the host's fold of the two status words flags some lanes, not all, and keys
    and status agree on every copy of a row."""
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
    monkeypatch.setenv("KG_SMALL_REPLICAS", replicas)
    try:
        keys, status = select_acc(snap, batch, monkeypatch, oracle_keys("marked", kc, marked, pods))
        assert np.array_equal(status, status[first]) and np.array_equal(keys, keys[first])
        assert not (status & ~np.uint32(abi.KG_ST_UNSUPPORTED)).any()
        assert 2 <= (status[:100] != 0).sum() < 100
    finally:
        batch.close()
        snap.close()


@pytest.mark.gpu
def test_big_records(gpu, monkeypatch):
    """24 adjacent F_BIG records: their workgroups' atomics arrive long after the others'."""
    from koordinator_amd import engine
    ctx = gpu[0]
    kc, sub = grouped_big()
    pods = tiled_small()
    snap = engine.Snapshot(ctx, kc, sub)
    batch = engine.PodBatch(ctx, pods)
    try:
        for _ in range(2):
            keys, _ = select_acc(snap, batch, monkeypatch, oracle_keys("grouped_big", kc, sub, pods))
        assert (keys != 0).any()
    finally:
        batch.close()
        snap.close()


# ---- 5: edges ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_no_feasible_node(gpu, monkeypatch):
    """A pod that fits no node adds nothing to any accumulator: key 0 and status 0 on its rows, twice in a row."""
    from koordinator_amd import engine
    ctx, snap, kc, nodes = gpu
    pods, lane = one_unfit()
    batch = engine.PodBatch(ctx, pods)
    try:
        want = oracle_keys("one_unfit", kc, nodes, pods)
        for _ in range(2):
            keys, status = select_acc(snap, batch, monkeypatch, want)
            assert not keys[lane == 2].any() and keys[lane != 2].all() and not status.any()
    finally:
        batch.close()


@pytest.mark.gpu
@pytest.mark.parametrize("replicas", ["1", None])
@pytest.mark.parametrize("lanes", [64, 65, 256])
def test_lane_counts(gpu, monkeypatch, lanes, replicas):
    """A full wave of lanes, one lane into the second wave (63 idle lanes add nothing) and the full block."""
    from koordinator_amd import engine
    ctx, snap, kc, nodes = gpu
    pods = fast_distinct(lanes)
    batch = engine.PodBatch(ctx, pods)
    if replicas:
        monkeypatch.setenv("KG_SMALL_REPLICAS", replicas)
    try:
        assert batch.select_lanes() == (lanes, lanes)
        for _ in range(2):
            keys, _ = select_acc(snap, batch, monkeypatch, oracle_keys(("small", lanes), kc, nodes, pods))
        assert (keys != 0).any()
    finally:
        batch.close()


@pytest.mark.gpu
def test_one_workgroup(gpu, monkeypatch):
    """Five records of one class: one workgroup, which also zeroes the whole dirty extent of the other parity."""
    from koordinator_amd import engine
    ctx, _, kc, nodes = gpu
    five = one_class_five(nodes)
    pods = tiled_small()
    snap = engine.Snapshot(ctx, kc, five)
    batch = engine.PodBatch(ctx, pods)
    try:
        want = oracle_keys("acc_five", kc, five, pods)
        for _ in range(3):
            keys, _ = select_acc(snap, batch, monkeypatch, want)
        assert (keys != 0).any()
    finally:
        batch.close()
        snap.close()


@pytest.mark.gpu
@pytest.mark.parametrize("chunks", ["1,1,1", "1,1,5"])
def test_more_workgroups_than_compute_units(gpu, monkeypatch, chunks):
    """One record per workgroup, 300 workgroups: some start when others have ended, and no one waits for another."""
    from koordinator_amd import engine
    ctx, snap, kc, nodes = gpu
    pods = tiled_small()
    batch = engine.PodBatch(ctx, pods)
    monkeypatch.setenv("KG_SMALL_CHUNKS", chunks)
    try:
        want = oracle_keys(("small", "tiled"), kc, nodes, pods)
        for _ in range(3):
            select_acc(snap, batch, monkeypatch, want)
    finally:
        batch.close()


@pytest.mark.gpu
def test_many_rows(gpu, monkeypatch, tmp_path):
    """40,000 rows of three pods: the launch does not depend on the row count. Its phase file (KG_SMALL_PHASES) keeps
    four readings per workgroup, the fourth from the one workgroup that drew the measurement aid's last ticket; the
    select after it finds the ticket back at zero."""
    from koordinator_amd import engine
    ctx, snap, kc, nodes = gpu
    n = 40000
    pods = three_pods(n)
    batch = engine.PodBatch(ctx, pods)
    try:
        assert batch.select_lanes() == (3, 3)
        want = oracle_keys("three", kc, nodes, fast_distinct(3))[np.arange(n) % 3]
        keys, status = select_acc(snap, batch, monkeypatch, want)
        assert (keys != 0).any() and not status.any()
        path = tmp_path / "acc.bin"
        monkeypatch.setenv("KG_SMALL_PHASES", str(path))
        for _ in range(2):
            got, st = read(snap, batch)
            assert np.array_equal(got, want) and not st.any()
        monkeypatch.delenv("KG_SMALL_PHASES")
        recs = phase_records(path)
        assert len(recs) == 2
        for r in recs:
            assert (r[:, 3] != 0).sum() == 1 and (r[:, :3] != 0).all()
            assert (r[:, 0] <= r[:, 1]).all() and (r[:, 1] <= r[:, 2]).all() and r[:, 3].max() >= r[:, 2].max()
        keys, _ = select_acc(snap, batch, monkeypatch, want)
    finally:
        batch.close()


# ---- 6: reads ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_reads(gpu, monkeypatch):
    """Status before keys and each read twice: one answer, folded once. A burst of 12 async selects and one read: the
    last launch's parity. After a later upload both reads fail with "no selection result"."""
    from koordinator_amd import engine
    ctx, snap, kc, nodes = gpu
    pods = shuffled37()
    want = oracle_keys("shuffled37", kc, nodes, pods)
    batch = engine.PodBatch(ctx, pods, capacity=2000)
    try:
        engine.eval_select_async(snap, batch, 1)
        status = engine.result_status(batch)
        assert not status.any() and np.array_equal(engine.result_status(batch), status)
        assert np.array_equal(engine.result_keys(batch, 1), want)
        assert np.array_equal(engine.result_keys(batch, 1), want)
        assert np.array_equal(engine.result_status(batch), status)
        for _ in range(12):
            engine.eval_select_async(snap, batch, 1)
        assert np.array_equal(engine.result_keys(batch, 1), want)
        assert np.array_equal(engine.result_status(batch), status)
        select_acc(snap, batch, monkeypatch, want)
        for later in (tiled(2000), tiled(5)):
            batch.upload(later)
            for call in (lambda: engine.result_keys(batch, 1), lambda: engine.result_status(batch)):
                with pytest.raises(engine.EngineError, match="no selection result") as e:
                    call()
                assert e.value.status == KG_INVALID_ARG
            m = abi.table_len(later)
            keys, status = select_acc(snap, batch, monkeypatch,
                                      oracle_keys("tiled_64", kc, nodes, tiled(64))[np.arange(m) % 64])
            assert not status.any()
    finally:
        batch.close()


# ---- 7: profiling ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("bound", [False, True])
def test_profiling(gpu, monkeypatch, bound):
    """Profiling on, with the device-clock slots and with the bound event pair: keys and status are those of profiling
    off, one launch is counted per select, and every synchronised select's bracket is positive and below the wall-clock
    time of that select (a begin or end word left by an earlier launch would give more)."""
    from koordinator_amd import engine
    ctx, snap, kc, nodes = gpu
    pods = shuffled37()
    batch = engine.PodBatch(ctx, pods)
    try:
        keys_off, status_off = select_acc(snap, batch, monkeypatch, oracle_keys("shuffled37", kc, nodes, pods))
        if bound:
            monkeypatch.setenv("KG_PROFILE_BOUND_EVENTS", "1")
        ctx.sync()
        ctx.profile(True)
        try:
            ctx.profile_read(reset=True)
            for _ in range(3):
                t0 = time.perf_counter()
                engine.eval_select_async(snap, batch, 1)
                ctx.sync()
                wall = (time.perf_counter() - t0) * 1e3
                ms, launches = ctx.profile_read(reset=True)
                print(f"bound {bound}: bracket {ms:.5f} ms, wall clock {wall:.5f} ms")
                assert launches == 1 and 0 < ms < wall, (ms, wall, launches)
                assert np.array_equal(engine.result_keys(batch, 1), keys_off)
                assert np.array_equal(engine.result_status(batch), status_off)
        finally:
            ctx.profile(False)
    finally:
        batch.close()


@pytest.mark.gpu
def test_profile_counting(gpu, monkeypatch):
    """This form mixed with row-form and top-3 selects: one launch counted per select, a read in between does not
    reset. Then more async selects than the slot table holds and one read: the select that finds the table full drains
    it, and the count is the burst's."""
    from koordinator_amd import engine
    ctx, snap, kc, nodes = gpu
    pods = shuffled37()
    want = oracle_keys("shuffled37", kc, nodes, pods)
    batch = engine.PodBatch(ctx, pods)
    try:
        ctx.profile(True)
        try:
            ctx.profile_read(reset=True)
            n = 0
            for round_ in range(2):
                for _ in range(2):
                    engine.eval_select_async(snap, batch, 1)
                engine.eval_select_async(snap, batch, 3)
                engine.eval_select_async(snap, batch, 1)
                monkeypatch.setenv("KG_SMALL_ROW_RESULTS", "1")
                engine.eval_select_async(snap, batch, 1)
                monkeypatch.delenv("KG_SMALL_ROW_RESULTS")
                engine.eval_select_async(snap, batch, 1)
                n += 6
                if round_ == 0:
                    ms1, launches1 = ctx.profile_read()
                    assert launches1 == 6 and ms1 > 0
            ms, launches = ctx.profile_read(reset=True)
            assert launches == n and ms > ms1
            assert np.array_equal(engine.result_keys(batch, 1), want)
            burst = PROF_SLOTS + 3
            for _ in range(burst):
                engine.eval_select_async(snap, batch, 1)
            ms, launches = ctx.profile_read(reset=True)
            assert launches == burst and ms > 0
            assert ctx.profile_read() == (0.0, 0)
            assert np.array_equal(engine.result_keys(batch, 1), want)
        finally:
            ctx.profile(False)
    finally:
        batch.close()
