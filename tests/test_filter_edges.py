"""Every device consumer of the Filter against the CPU oracle on the edge lattice of filter_edges.py: each predicate
on, one below and one above its threshold, over capacities on both sides of the float64 fast path. The oracle itself
is pinned on the same lattice by test_filter_ref.py (an independent restatement from the Go sources).

Consumers: kg_eval_verify; the select on its fast and integer paths (every pair, through 4-node snapshots whose top-4
keys show all four totals); the one-launch top-1 select and the general top-1 (whole lattice and one-node snapshots,
where the key alone is the verdict); kg_eval_feasible, kg_eval_diagnose and kg_eval_offer_slots; the replay, Assume /
Forget and row updates, where the heads later pods meet come from the device's own derive_node.

Bar: exact equality everywhere."""
import functools

import numpy as np
import pytest

import filter_edges as fe
import filter_ref
import offer_slots_ref
import oracle_lib
from koordinator_amd import abi, engine, nodesets, synth
from test_diagnose import expected as diag_expected
from test_gpu_parity import assert_verify_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def lat():
    """(kc, nodes, pods, cells, index of pod keys, the oracle's verify result) of the lattice; read-only."""
    cfg, nodes, pods, cells = fe.lattice()
    kc = cfg.kg_config()
    return kc, nodes, pods, cells, fe.pod_table()[1], oracle_lib.eval_verify(kc, nodes, pods)


def fast_rows(pods):
    """The pods inside the fast value domain (every pod but the estimates past 2^44)."""
    return np.flatnonzero((pods["la_est0"] < fe.BIG_EST) & (pods["la_est1"] < fe.BIG_EST))


def small_rows(pods):
    """fe.small_rows: at most 256 lanes, a whole wave of each kind, every tuned pod of the fast domain."""
    return fe.small_rows(pods, fe.pod_table()[1])


def cell_of(cells, name, cap, form, delta):
    hits = [i for i, (p, d, _) in enumerate(cells) if (p.name, p.cap, p.form, d) == (name, cap, form, delta)]
    assert hits, (name, cap, form, delta)
    return hits[0]


def want_keys(total, idx, base=0):
    """The oracle's top-1 keys of the pods over the nodes idx (snapshot positions base + t) from its totals."""
    out = np.zeros(total.shape[0], np.uint64)
    for t in reversed(range(len(idx))):  # the lowest position wins a tie
        col = total[:, idx[t]]
        key = np.array([abi.make_key(v, base + t) if v >= 0 else 0 for v in col], np.uint64)
        out = np.where(key >= out, key, out)
    return out


# ---- verify -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ignored,filter_expired,schedule_expired", [(0, 1, 0), (3, 1, 1), (1, 0, 0), (2, 0, 1)])
def test_verify(ctx, ignored, filter_expired, schedule_expired):
    _, nodes, pods, cells, _, _ = lat()
    kc = synth.bench_profile(numa=True).kg_config()
    kc.nrf_ignored_scalars, kc.la_filter_expired, kc.la_schedule_expired = ignored, filter_expired, schedule_expired
    snap, batch = engine.Snapshot(ctx, kc, nodes), engine.PodBatch(ctx, pods)
    try:
        ref = oracle_lib.eval_verify(kc, nodes, pods)
        assert_verify_equal(engine.eval_verify(snap, batch), ref, f"lattice {ignored} {filter_expired} {schedule_expired}")
        for i, cell in enumerate(cells):  # the tuned pairs say what the cells say
            assert int(ref.status[cell[2], i]) == fe.expected_word(kc, cell, nodes, i, pods) or \
                (ignored and cell[0].name in ("nrf_sc0", "nrf_sc1")), cell
    finally:
        batch.close()
        snap.close()


# ---- select, every pair -------------------------------------------------------------------------------------------------

def groups_of_four(nodes):
    """Groups all of storage class 0, all of class 1 (SingleNUMANode) and mixed; together they hold every node."""
    single = nodes["numa_policy"] == abi.KG_NUMA_SINGLE_NODE
    c0, c1 = np.flatnonzero(~single), np.flatnonzero(single)
    out = [c0[g:g + 4] for g in range(0, len(c0), 4)] + [c1[g:g + 4] for g in range(0, len(c1), 4)]
    for t in range(0, len(c1) - 1, 2):
        out.append(np.array([c1[t], c0[3 * t], c0[3 * t + 1], c1[t + 1]]))
    return out


@pytest.mark.parametrize("path", [None, "KG_SELECT_INT"])
def test_select_every_pair(ctx, monkeypatch, path):
    """Key 0 <=> infeasible, and the totals, of every pair: whole batch (the kind-specialised loops run whole waves)
    on the fast path and with every lane forced onto the integer path."""
    kc, nodes, pods, cells, _, ref = lat()
    if path:
        monkeypatch.setenv(path, "1")
    batch = engine.PodBatch(ctx, pods)
    n_fast = len(fast_rows(pods))
    got = np.full(ref.total.shape, -2, np.int64)
    try:
        assert batch.select_lanes() == (abi.table_len(pods), n_fast)
        for idx in groups_of_four(nodes):
            snap = engine.Snapshot(ctx, kc, abi.take(nodes, idx))
            assert batch.fast_lanes(snap) == (0 if path else n_fast)
            keys = engine.eval_select(snap, batch, 4)
            assert not engine.result_status(batch).any()
            sub = np.full((keys.shape[0], len(idx)), -1, np.int64)
            for t in range(4):
                nz = keys[:, t] != 0
                sub[np.flatnonzero(nz), abi.key_node(keys[nz, t])] = abi.key_total(keys[nz, t])
            snap.close()
            bad = np.argwhere(sub != ref.total[:, idx])
            assert not len(bad), (path, [(int(j), int(idx[t]), cells[idx[t]], int(sub[j, t]), int(ref.total[j, idx[t]]))
                                         for j, t in bad[:4]])
            got[:, idx] = sub
        assert np.array_equal(got, ref.total)
        assert np.array_equal(got < 0, ref.status != 0)
    finally:
        batch.close()


# ---- top-1: the one-launch select and the general one ---------------------------------------------------------------------

def top1_both(snap, batch, monkeypatch):
    """(keys, status) of the one-launch select (its F_BIG gate lifted: the lattice is a third F_BIG) after checking that
    the general top-1 gives the same."""
    monkeypatch.setenv("KG_SMALL_ALLOW_BIG", "1")
    keys, status = engine.eval_select(snap, batch, 1)[:, 0], engine.result_status(batch)
    monkeypatch.delenv("KG_SMALL_ALLOW_BIG")
    monkeypatch.setenv("KG_NO_SMALL_SELECT", "1")
    keys0, status0 = engine.eval_select(snap, batch, 1)[:, 0], engine.result_status(batch)
    monkeypatch.delenv("KG_NO_SMALL_SELECT")
    assert np.array_equal(keys, keys0) and np.array_equal(status, status0)
    return keys, status


def test_top1_whole_lattice(ctx, monkeypatch):
    kc, nodes, pods, cells, _, ref = lat()
    rows = small_rows(pods)
    sub = abi.take(pods, rows)
    snap = engine.Snapshot(ctx, kc, nodes, index_base=3)
    batch, whole = engine.PodBatch(ctx, sub), engine.PodBatch(ctx, pods)
    try:
        assert batch.select_lanes() == (len(rows), len(rows)) and len(rows) <= 256
        keys, status = top1_both(snap, batch, monkeypatch)
        assert np.array_equal(keys, oracle_lib.select(kc, nodes, sub, 1, index_base=3)[:, 0])
        assert not status.any()
        # with the integer lanes of the large estimates: the general path
        assert np.array_equal(engine.eval_select(snap, whole, 1), oracle_lib.select(kc, nodes, pods, 1, index_base=3))
        assert not engine.result_status(whole).any()
    finally:
        batch.close()
        whole.close()
        snap.close()


def test_top1_one_node_snapshots(ctx, monkeypatch):
    """One node: the key alone shows the verdict. The delta 0 and +1 cells of every predicate and the 25 float points."""
    kc, nodes, pods, cells, _, ref = lat()
    rows = small_rows(pods)
    batch = engine.PodBatch(ctx, abi.take(pods, rows))
    picks = fe.subsample(cells)
    assert 50 <= len(picks) <= 70
    try:
        for i in picks:
            snap = engine.Snapshot(ctx, kc, abi.take(nodes, [i]), index_base=i)
            keys, status = top1_both(snap, batch, monkeypatch)
            snap.close()
            want = want_keys(ref.total[rows], [i], base=i)
            assert np.array_equal(keys, want), (cells[i], np.flatnonzero(keys != want)[:5])
            assert not status.any()
            j = cells[i][2]
            if j in rows:  # the tuned pod: feasible exactly when the cell passes
                t = int(np.flatnonzero(rows == j)[0])
                assert (keys[t] != 0) == (fe.expected_word(kc, cells[i], nodes, i, pods) == 0), cells[i]
    finally:
        batch.close()


# ---- feasible bitmaps, diagnosis ------------------------------------------------------------------------------------------

def test_feasible_and_diagnose(ctx):
    kc, nodes, pods, cells, _, ref = lat()
    n = abi.table_len(nodes)
    snap, batch = engine.Snapshot(ctx, kc, nodes), engine.PodBatch(ctx, pods)
    try:
        for mask in (0xFFFFFFFF, abi.KG_ST_UNRESOLVABLE_MASK, abi.KG_ST_LA_MASK, abi.KG_ST_NRF_MASK | abi.KG_ST_NUMA_MASK):
            bits, cnt = engine.eval_feasible(snap, batch, fail_mask=mask, counts=True)
            want = (ref.status & np.uint32(mask)) == 0
            got = nodesets.to_mask(bits, n)
            assert np.array_equal(got, want), (hex(mask), np.argwhere(got != want)[:5])
            assert np.array_equal(cnt, want.sum(axis=1).astype(np.uint32))
        for first_plugin in (True, False):
            got = engine.eval_diagnose(snap, batch, first_plugin=first_plugin)
            assert np.array_equal(got, diag_expected(ref.status, first_plugin)), first_plugin
    finally:
        batch.close()
        snap.close()


# ---- nodes with room for exactly m pods -----------------------------------------------------------------------------------

X = 1000  # the size of the pods below: fe.SIZES[2]
BRIM = {"nrf_cpu": ("prod", abi.KG_ST_NRF_CPU), "nrf_mem": ("gen", abi.KG_ST_NRF_MEM), "nrf_eph": ("batch", abi.KG_ST_NRF_EPH),
        "nrf_sc0": ("batch", abi.KG_ST_NRF_SC0), "nrf_sc1": ("gen", abi.KG_ST_NRF_SC1), "nrf_pods": ("prod", abi.KG_ST_NRF_PODS),
        "la_cpu": ("gen", abi.KG_ST_LA_CPU), "la_mem_prod": ("prod", abi.KG_ST_LA_MEM),
        "la_cpu_agg": ("batch", abi.KG_ST_LA_CPU | abi.KG_ST_LA_AGG), "amp": ("prod", abi.KG_ST_NUMA_AMP_CPU),
        "zone_cpu": ("prod", abi.KG_ST_NUMA_ALIGN), "zone_mem": ("gen", abi.KG_ST_NUMA_UNSATISFIED)}


def brim_node(name, m):
    """A node with room for exactly m pods of size X under the predicate (wide room under every other)."""
    n = fe.roomy_node()
    if name in fe.NRF_RES:
        a, u, _, _ = fe.NRF_RES[name]
        n[a], n[u] = 96000, 96000 - m * X
        if name in ("nrf_cpu", "nrf_mem"):
            n["nz" + u[3:]] = n[u]
    elif name == "nrf_pods":
        n.update(alloc_pods=10, num_pods=10 - m)
    elif name.startswith("la_"):  # m estimates that sum exactly to the cut-off
        r = 0 if "cpu" in name else 1
        prof = "prod" if name.endswith("prod") else "agg" if name.endswith("agg") else "usage"
        fe.set_la(n, r, prof, 96000, 65, filter_ref.la_cut(96000, 65) - m * X)
        if prof == "usage":
            n[f"la_fbase_prod{r}"] = n[f"la_sbase_prod{r}"] = 0
    elif name == "amp":  # requested - cpuset + Amplify(cpuset) + m X = allocatable, NodeResourcesFit still with room
        n.update(alloc_cpu=96000, cpu_amp_ratio=1.5, cpuset_alloc_milli=4000, req_cpu=96000 - m * X - 2000)
        n["nz_cpu"] = n["req_cpu"]
    elif name == "zone_cpu":  # zone 0 one unit short; zone 1 holds m pods and is then one unit short too
        n.update(numa_policy=abi.KG_NUMA_SINGLE_NODE, zone_cpu0=96000, zone_cpu1=96000, zone_cpu_used0=96000 - (X - 1),
                 zone_cpu_used1=96000 - (m * X + X - 1))
    elif name == "zone_mem":  # zone 0 full; zone 1 holds exactly m pods
        n.update(numa_policy=abi.KG_NUMA_SINGLE_NODE, zone_mem0=96000, zone_mem1=96000, zone_mem_used0=96000,
                 zone_mem_used1=96000 - m * X)
    else:
        raise ValueError(name)
    return n


def test_offer_slots(ctx):
    """Room for exactly m copies of a pod under one NodeResourcesFit predicate: the count is m, the first failing word
    the predicate's bit."""
    kc, _, pods, _, ix, _ = lat()
    names = list(fe.NRF_RES) + ["nrf_pods"]
    cases = [(name, m) for name in names for m in (0, 1, 3)]
    nodes = fe.node_table([brim_node(name, m) for name, m in cases])
    snap, batch = engine.Snapshot(ctx, kc, nodes), engine.PodBatch(ctx, pods)
    try:
        for kind in ("prod", "batch", "gen"):
            j = ix[(kind, 2, 0)]
            rows = np.full(5, j, np.uint32)
            slots, word = engine.eval_offer_slots(snap, batch, rows, status=True)
            ws, ww = offer_slots_ref.offer_slots(kc, nodes, pods, rows)
            assert np.array_equal(slots, ws) and np.array_equal(word, ww), kind
            for t, (name, m) in enumerate(cases):
                if kind in fe.REACH[name]:
                    bit = abi.KG_ST_NRF_PODS if name == "nrf_pods" else fe.NRF_RES[name][3]
                    assert (int(slots[t]), int(word[t])) == (m, bit), (kind, name, m)
                elif name != "nrf_pods":
                    assert (int(slots[t]), int(word[t])) == (5, 0), (kind, name, m)
    finally:
        batch.close()
        snap.close()


@pytest.mark.parametrize("mode", ["window", "step"])
@pytest.mark.parametrize("name", list(BRIM))
def test_replay_to_the_brim(ctx, monkeypatch, mode, name):
    """A one-node snapshot sized for exactly m pods, m + 1 copies replayed: the first m are placed, the last gets the
    predicate's reason; the heads it meets are the device's derive_node after each Assume."""
    if mode == "step":
        monkeypatch.setenv("KG_REPLAY_STEP", "1")
    kc, _, pods, _, ix, _ = lat()
    kind, bit = BRIM[name]
    m = 3
    nodes = fe.node_table([brim_node(name, m)])
    copies = abi.take(pods, [ix[(kind, 2, 0)]] * (m + 1))
    snap, batch = engine.Snapshot(ctx, kc, nodes, index_base=5), engine.PodBatch(ctx, copies)
    try:
        node, total, reason = engine.replay(snap, batch, reasons=True)
        st = oracle_lib.OracleState(kc, nodes)
        want_node, want_total, want_reason = st.replay(copies, index_base=5, reasons=True)
        assert node.tolist() == [5] * m + [-1], (name, node)
        assert int(reason[m]) == bit and not reason[:m].any(), (name, [hex(int(x)) for x in reason])
        assert np.array_equal(node, want_node) and np.array_equal(total, want_total)
        assert np.array_equal(reason, want_reason)
        got_state, want_state = snap.read_state(), st.table()
        for k, v in got_state.items():
            assert np.array_equal(v, want_state[k]), (name, k)
    finally:
        batch.close()
        snap.close()


# ---- Assume / Forget, row updates -------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,form", [("nrf_cpu", ""), ("nrf_sc1", ""), ("nrf_pods", ""), ("la_cpu", "usage"),
                                       ("amp", "1.5x1000"), ("zone_cpu", "only1"), ("zone_mem", "only1")])
def test_assume_then_forget(ctx, name, form):
    """Assume of the exactly-fitting pod makes the next select infeasible for it; Forget brings back the select of
    before, key for key."""
    kc, nodes, pods, cells, _, ref = lat()
    i = cell_of(cells, name, 96000, form, 0)
    j = cells[i][2]
    one = abi.take(nodes, [i])
    rows = small_rows(pods)
    sub = abi.take(pods, rows)
    t = int(np.flatnonzero(rows == j)[0])
    snap, batch = engine.Snapshot(ctx, kc, one), engine.PodBatch(ctx, sub)
    try:
        before = engine.eval_select(snap, batch, 1)
        assert np.array_equal(before[:, 0], want_keys(ref.total[rows], [i])) and before[t, 0] != 0
        zone = int(ref.numa_zone[j, i])
        engine.assume(snap, batch, t, 0)
        st = oracle_lib.OracleState(kc, one)
        assert st.assume(0, sub, t)
        after = engine.eval_select(snap, batch, 1)
        assert np.array_equal(after, oracle_lib.select(kc, merged(one, st.table()), sub, 1))
        assert after[t, 0] == 0
        assert_verify_equal(engine.eval_verify(snap, batch), oracle_lib.eval_verify(kc, merged(one, st.table()), sub), name)
        engine.forget(snap, batch, t, 0, zone)
        assert np.array_equal(engine.eval_select(snap, batch, 1), before)
    finally:
        batch.close()
        snap.close()


def merged(nodes, state):
    """The node table with the oracle state's columns."""
    out = dict(nodes)
    out.update({k: v for k, v in state.items() if k in nodes})
    return out


def shifted_total(total, thr):
    """A LoadAware total just below `total` whose cut-off is the cut-off of `total` minus 1."""
    cut = filter_ref.la_cut(total, thr)
    for t in range(total - 1, total - 50, -1):
        if filter_ref.la_cut(t, thr) == cut - 1:
            return t
    raise AssertionError("no such total")


@pytest.mark.parametrize("what", ["la_alloc", "la_thr", "req_cpu"])
def test_update_rows(ctx, monkeypatch, what):
    """A delta 0 node moved to delta +1 and back by a row update: of the LoadAware total or threshold alone (the cut-off
    is found again at the update), or of the node's requested cpu alone. Verify and both top-1 selects follow."""
    kc, nodes, pods, cells, _, ref = lat()
    if what == "req_cpu":
        i = cell_of(cells, "nrf_cpu", 96000, "", 0)
        bit = abi.KG_ST_NRF_CPU
    else:
        i = cell_of(cells, "la_cpu", 96000, "usage", 0)
        bit = abi.KG_ST_LA_CPU
    j = cells[i][2]
    rows = small_rows(pods)
    sub = abi.take(pods, rows)
    t = int(np.flatnonzero(rows == j)[0])
    one = abi.take(nodes, [i])
    moved = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in one.items()}
    if what == "req_cpu":
        moved["req_cpu"][0] += 1
    elif what == "la_alloc":
        moved["la_alloc0"][0] = shifted_total(int(one["la_alloc0"][0]), int(one["la_thr_usage0"][0]))
    else:
        moved["la_thr_usage0"][0] -= 1
    snap, batch = engine.Snapshot(ctx, kc, one), engine.PodBatch(ctx, sub)
    try:
        for step, table in enumerate((one, moved, one, moved)):
            if step:
                snap.update_rows([0], table)
            want = oracle_lib.eval_verify(kc, table, sub)
            assert int(want.status[t, 0]) == (bit if table is moved else 0), (what, step)
            assert_verify_equal(engine.eval_verify(snap, batch), want, f"{what} step {step}")
            keys, _ = top1_both(snap, batch, monkeypatch)
            assert np.array_equal(keys, want_keys(want.total, [0])), (what, step)
            assert (keys[t] == 0) == (table is moved)
    finally:
        batch.close()
        snap.close()
