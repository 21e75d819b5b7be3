"""Select, verify and replay against the CPU oracle, bit-exact, across the scoring configuration space: base plugin
masks 1..6, per-resource weights on the fast path's weighted means (weighted_boundary.py puts the means on and next to
integers), configurations past the fast path's weight domain, plugin weights up to 2^20, and the ext plugins' weights.
test_score_ref.py checks the oracle itself against an independent restatement on the same clusters and asserts the
residue conditions; the configurations are config_cases.py's."""
import numpy as np
import pytest

import config_cases as cc
import oracle_lib
import weighted_boundary as wb
from koordinator_amd import abi, engine, synth
from test_gpu_parity import _all_totals_via_select, assert_verify_equal
from test_pod_dedup import distinct_rows, wave_kind

pytestmark = pytest.mark.gpu

PATHS = (None, "KG_NO_SMALL_SELECT", "KG_NO_POD_DEDUP", "KG_NO_IPRUNE", "KG_SELECT_INT")
NRF, LA, NUMA = abi.KG_PLUGIN_NRF, abi.KG_PLUGIN_LA, abi.KG_PLUGIN_NUMA


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    yield c
    c.close()


def copy(t):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in t.items()}


def vbig_cluster():
    cfg, nodes, pods = synth.small(600, 300, seed=41, numa=True)
    nodes = copy(nodes)
    nodes["alloc_mem"][::37] = 1 << 50  # F_VBIG: outside the fast value domain, never pruned
    nodes["la_alloc1"][5::41] = 1 << 50
    return cfg, nodes, pods, np.zeros(0, np.int64)


def decoy_cluster(mask):
    """synth.mixed(600, 300) with pods carrying a NUMA policy of their own, and 12 decoys: F_BIG records inside the fast
    value domain (Restricted / BestEffort policies), emptied so that they score best, which fail exactly the plugins
    `mask` disables: over the LoadAware threshold, "Too many pods" (NodeResourcesFit; the zones keep their room), every
    zone full (NodeNUMAResource; Restricted nodes)."""
    cfg, nodes, pods = synth.mixed(600, 300, seed=43)
    nodes, pods = copy(nodes), copy(pods)
    rng = np.random.default_rng(43)
    own = rng.random(300) < 0.12
    pods["numa_policy"] = np.where(own, rng.choice([abi.KG_NUMA_BEST_EFFORT, abi.KG_NUMA_RESTRICTED,
                                                     abi.KG_NUMA_SINGLE_NODE], 300), pods["numa_policy"]).astype(np.uint32)
    pol = nodes["numa_policy"]
    pick = np.flatnonzero((pol == abi.KG_NUMA_RESTRICTED) if not mask & NUMA else
                          ((pol == abi.KG_NUMA_RESTRICTED) | (pol == abi.KG_NUMA_BEST_EFFORT)))
    # past the integer lanes' 256 seed records (k_int_seed evaluates those in full, k_int_filter prunes the rest). The
    # device order is class 0 ascending, then class 1 (SingleNUMANode nodes): a Restricted / BestEffort node sits at
    # least as far in as the nodes of another policy than SingleNUMANode before it
    place = np.cumsum(pol != abi.KG_NUMA_SINGLE_NODE) - 1
    decoys = pick[place[pick] >= 256][:12]
    assert len(decoys) == 12
    for col in ("req_cpu", "req_mem", "req_eph", "nz_cpu", "nz_mem", "sc_req0", "sc_req1", "num_pods", "cpuset_alloc_milli",
                "la_sbase_np0", "la_sbase_np1", "la_sbase_prod0", "la_sbase_prod1", "la_fbase_np0", "la_fbase_np1",
                "la_fbase_prod0", "la_fbase_prod1", "numa_zone_status"):
        nodes[col][decoys] = 0
    nodes["cpu_alloc"][decoys] = 0
    nodes["la_flags"][decoys] = abi.KG_LA_HAS_METRIC
    for z in range(abi.KG_MAX_ZONES):
        nodes[f"zone_cpu_used{z}"][decoys] = 0
        nodes[f"zone_mem_used{z}"][decoys] = 0
    if not mask & LA:
        for r in range(2):
            nodes[f"la_fbase_np{r}"][decoys] = nodes[f"la_alloc{r}"][decoys]
            nodes[f"la_fbase_prod{r}"][decoys] = nodes[f"la_alloc{r}"][decoys]
    if not mask & NRF:
        nodes["num_pods"][decoys] = nodes["alloc_pods"][decoys]
    if not mask & NUMA:
        for z in range(abi.KG_MAX_ZONES):
            nodes[f"zone_cpu_used{z}"][decoys] = nodes[f"zone_cpu{z}"][decoys]
            nodes[f"zone_mem_used{z}"][decoys] = nodes[f"zone_mem{z}"][decoys]
    return cfg, nodes, pods, decoys


def run_paths(ctx, kc, nodes, pods, monkeypatch, ks=(1, 4), paths=PATHS, what="", fast=True):
    """fast: whether the configuration is inside the fast path's weight domain. Which path a launch takes is read
    from the engine (fast_lanes: the batch's fast lanes on this snapshot): some without a switch when `fast`, none
    under KG_SELECT_INT=1 or when not `fast`."""
    snap = engine.Snapshot(ctx, kc, nodes, index_base=11)
    batch = engine.PodBatch(ctx, pods)
    try:
        assert batch.select_lanes()[1] > 0  # the pods themselves are fast-lane material
        ref = oracle_lib.eval_verify(kc, nodes, pods)
        assert_verify_equal(engine.eval_verify(snap, batch), ref, what)
        unsup = np.bitwise_or.reduce(ref.status & abi.KG_ST_UNSUPPORTED, axis=1)
        want = {k: oracle_lib.select(kc, nodes, pods, k, index_base=11) for k in ks}
        for path in paths:
            if path:
                monkeypatch.setenv(path, "1")
            want_fast = batch.select_lanes()[1] if fast and path != "KG_SELECT_INT" else 0
            assert batch.fast_lanes(snap) == want_fast, (what, path)
            for k in ks:
                got = engine.eval_select(snap, batch, k)
                bad = np.flatnonzero((got != want[k]).any(axis=1))
                assert not len(bad), (f"{what} {path or 'default'} k={k}: {len(bad)} pods differ, first {bad[0]}: "
                                      f"gpu={got[bad[0]]} oracle={want[k][bad[0]]}")
                if not unsup.any():
                    assert not engine.result_status(batch).any(), (what, path, k)
            if path:
                monkeypatch.delenv(path)
        return want
    finally:
        batch.close()
        snap.close()


@pytest.mark.parametrize("mask", [1, 2, 3, 4, 5, 6])
def test_plugin_masks_vbig(ctx, monkeypatch, mask):
    cfg, nodes, pods, _ = vbig_cluster()
    kc = cfg.kg_config()
    kc.plugins = mask
    want = run_paths(ctx, kc, nodes, pods, monkeypatch, what=f"mask {mask}")
    assert (want[1] != 0).any()


def decoy_winners(kc, nodes, pods, decoys, mask):
    kc7 = cc.only(cc.bench_profile(), 7)
    top = abi.key_node(oracle_lib.select(kc, nodes, pods, 1)[:, 0])
    top7 = abi.key_node(oracle_lib.select(kc7, nodes, pods, 1)[:, 0])
    feas = oracle_lib.select(kc, nodes, pods, 1)[:, 0] != 0
    return np.flatnonzero(feas & np.isin(top, decoys) & ~np.isin(top7, decoys))


@pytest.mark.parametrize("mask", [1, 2, 3, 4, 5, 6])
def test_plugin_masks_decoys(ctx, monkeypatch, mask):
    """F_BIG records that are the best choice and fail only a disabled plugin: every prune must keep them."""
    cfg, nodes, pods, decoys = decoy_cluster(mask)
    kc = cfg.kg_config()
    kc.plugins = mask
    win = decoy_winners(kc, nodes, pods, decoys, mask)
    lanes = np.array([wave_kind(pods, int(j)) for j in win])
    print(f"mask {mask}: {len(win)} pods win a decoy, {int((lanes == 3).sum())} of them integer lanes")
    assert len(win) >= 8
    if mask & NUMA:  # without NodeNUMAResource no pod is an integer lane for its policy
        assert (lanes == 3).sum() >= 1 and (lanes < 3).sum() >= 1
    run_paths(ctx, kc, nodes, pods, monkeypatch, what=f"mask {mask}")


@pytest.mark.parametrize("mask", [4, 5, 6])
def test_plugin_masks_one_launch(ctx, monkeypatch, mask):
    """At most 256 distinct fast lanes at top-1: the one-launch select (its inline F_BIG prune), told as
    test_small_select.py tells it: the launch's lane counts, with the F_BIG share gate lifted."""
    cfg, nodes, pods, decoys = decoy_cluster(mask)
    fast = np.array([j for j in range(300) if wave_kind(pods, j) < 3][:200])
    sub = abi.take(pods, fast)
    kc = cfg.kg_config()
    kc.plugins = mask
    assert len(decoy_winners(kc, nodes, sub, decoys, mask)) >= 8
    snap = engine.Snapshot(ctx, kc, nodes)
    batch = engine.PodBatch(ctx, sub)
    try:
        n = distinct_rows(sub)
        assert batch.select_lanes() == (n, n) and n <= 256
        monkeypatch.setenv("KG_SMALL_ALLOW_BIG", "1")
        got = engine.eval_select(snap, batch, 1)
        assert np.array_equal(got, oracle_lib.select(kc, nodes, sub, 1))
    finally:
        batch.close()
        snap.close()


WEIGHT_CASES = cc.weight_cases()


@pytest.mark.parametrize("name,cfg,means", WEIGHT_CASES, ids=[c[0] for c in WEIGHT_CASES])
def test_weighted_means_on_boundaries(ctx, name, cfg, means):
    """Every pair's total on the boundary cluster through 4-node snapshots at top-4, then whole-cluster selects."""
    nodes, pods, _, _ = wb.cluster(cfg, seed=31)
    kc = cfg.kg_config()
    want = oracle_lib.eval_verify(kc, nodes, pods)
    assert (want.total >= 0).mean() > 0.2
    got = _all_totals_via_select(ctx, kc, nodes, pods)
    bad = np.argwhere(got != want.total)
    assert len(bad) == 0, (f"{len(bad)} totals differ, first {bad[0]}: gpu={got[tuple(bad[0])]} "
                           f"oracle={want.total[tuple(bad[0])]}")
    snap = engine.Snapshot(ctx, kc, nodes)
    batch = engine.PodBatch(ctx, pods)
    try:
        for k in (1, 4):
            assert np.array_equal(engine.eval_select(snap, batch, k), oracle_lib.select(kc, nodes, pods, k)), k
    finally:
        batch.close()
        snap.close()


SWITCH_CASES = cc.switch_cases()


@pytest.mark.parametrize("name,cfg", SWITCH_CASES, ids=[c[0] for c in SWITCH_CASES])
def test_past_the_fast_weight_domain(ctx, monkeypatch, name, cfg):
    """Weights above 4096, a LoadAware weight sum above 4096, MostAllocated strategies and ignored scalars send every
    lane to the integer path (run_paths reads that from the engine: no fast lane on these snapshots, for pods that are
    fast lanes elsewhere); on the boundary cluster too, where a float mean would be at its edge."""
    _, nodes, pods = synth.mixed(600, 300, seed=47)
    kc = cfg.kg_config()
    run_paths(ctx, kc, nodes, pods, monkeypatch, paths=(None, "KG_NO_IPRUNE"), what=name, fast=False)
    bn, bp, _, _ = wb.cluster(cfg, seed=33)
    run_paths(ctx, kc, bn, bp, monkeypatch, paths=(None,), what=name + " boundary", fast=False)


def test_plugin_weight_2p20_all_integer(ctx, monkeypatch):
    cfg = cc.with_plugin_weights(cc.with_nrf(cc.bench_profile(), (1 << 20, 1, 1, 1)), (1 << 20, 1 << 20, 1 << 20))
    _, nodes, pods = synth.small(400, 260, seed=49, numa=True)
    want = run_paths(ctx, cfg.kg_config(), nodes, pods, monkeypatch, paths=(None, "KG_SELECT_INT"), what="2^20",
                     fast=False)
    assert abi.key_total(want[1][:, 0]).max() > 100 << 20


@pytest.mark.parametrize("field,value", [("weight_nrf", (1 << 20) + 1), ("weight_numa", -1), ("nrf_w_mem", (1 << 20) + 1),
                                         ("la_dominant_w", -1), ("numa_hint_w_cpu", (1 << 20) + 1)])
def test_invalid_weights_are_refused(ctx, field, value):
    cfg, nodes, _ = synth.small(8, 1, seed=1)
    kc = cfg.kg_config()
    setattr(kc, field, value)
    with pytest.raises(engine.EngineError) as e:
        engine.Snapshot(ctx, kc, nodes)
    assert e.value.status == abi.KG_INVALID_ARG


@pytest.mark.parametrize("field", ["weight_dev", "weight_rsv"])
def test_invalid_ext_weights_are_refused(ctx, field):
    """An ext mask checks the ext weights too. (Σ plugin weights x 100 >= 2^31 cannot be reached with five weights of
    at most 2^20 each, 5 x 2^20 x 100 < 2^29.4: the bound on each weight is the check that fires.)"""
    cfg, nodes, pods, quotas, rsv = synth.cluster5(16, 4, seed_config=3)
    kc = cfg.kg_config()
    setattr(kc, field, (1 << 20) + 1)
    with pytest.raises(engine.EngineError) as e:
        engine.Snapshot(ctx, kc, nodes)
    assert e.value.status == abi.KG_INVALID_ARG


def replay_cfg(which):
    if which == "heavy":
        return cc.heavy().kg_config()
    kc = cc.bench_profile().kg_config()
    kc.plugins = int(which)
    return kc


@pytest.mark.parametrize("mode", ["window", "step"])
@pytest.mark.parametrize("which", ["3", "5", "heavy"])
def test_replay(ctx, monkeypatch, mode, which):
    if mode == "step":
        monkeypatch.setenv("KG_REPLAY_STEP", "1")
    _, nodes, pods = synth.small(300, 700, seed=51, scale=10.0)
    kc = replay_cfg(which)
    snap = engine.Snapshot(ctx, kc, nodes, index_base=3)
    batch = engine.PodBatch(ctx, pods)
    try:
        node, total = engine.replay(snap, batch)
        st = oracle_lib.OracleState(kc, nodes)
        want_node, want_total = st.replay(pods, index_base=3)
        assert np.array_equal(node, want_node)
        assert np.array_equal(total, want_total)
        assert (node < 0).any() and (node >= 0).any()  # the cluster fills up
        got_state, want_state = snap.read_state(), st.table()
        for k, v in got_state.items():
            assert np.array_equal(v, want_state[k]), k
    finally:
        batch.close()
        snap.close()


def ext_cfgs():
    out = []
    for wd, wr in ((1, 5000), (7, 3), (1000, 0), (0, 5000)):
        c = cc.config5()
        c.weight_dev, c.weight_rsv = wd, wr
        out.append((f"dev{wd}_rsv{wr}", c))
    for a, b in ((1, 1), (0, 3), (4, 1)):
        c = cc.config5()
        c.dev_scoring = [(n, w) for n, w in ((cc.GPU_MEMORY_RATIO, a), (cc.GPU_MEMORY, b)) if w]
        out.append((f"devw{a}_{b}", c))
    c = cc.config5()
    c.dev_strategy = "MostAllocated"
    out.append(("dev_most", c))
    return out


EXT_CASES = ext_cfgs()


@pytest.fixture(scope="module")
def ext_cluster():
    return synth.cluster5(300, 200, seed_config=53, rsv_frac=0.3)


@pytest.mark.parametrize("name,cfg", EXT_CASES, ids=[c[0] for c in EXT_CASES])
def test_ext_weights(ctx, ext_cluster, name, cfg):
    _, nodes, pods, quotas, rsv = ext_cluster
    kc = cfg.kg_config()
    snap = engine.Snapshot(ctx, kc, nodes)
    snap.upload_quotas(quotas)
    snap.upload_reservations(rsv)
    batch = engine.PodBatch(ctx, pods)
    try:
        for k in (1, 4):
            want = oracle_lib.ext_select(kc, nodes, pods, k, 0, quotas, rsv)
            assert np.array_equal(engine.eval_select(snap, batch, k), want), k
            assert (want != 0).any()
    finally:
        batch.close()
        snap.close()
    # replay without Reservation, as test_ext_parity.py's replay: placements, totals, GPU minors and quota use
    # (weight_rsv plays no part here: the selects above are what exercises it)
    kc.plugins &= ~abi.KG_PLUGIN_RSV
    snap = engine.Snapshot(ctx, kc, nodes)
    snap.upload_quotas(quotas)
    batch = engine.PodBatch(ctx, pods)
    try:
        node, total = engine.replay(snap, batch)
        minors = engine.replay_minors(batch)
        ost = oracle_lib.OracleState(kc, nodes)
        onode, ototal, ominors, oused, onp = ost.ext_replay(pods, quotas)
        assert np.array_equal(node, onode) and np.array_equal(total, ototal) and np.array_equal(minors, ominors)
        assert np.array_equal(snap.read_state()["dev_free"], ost.dev_free())
        used, _, npu, _ = snap.read_quotas()
        assert np.array_equal(used, oused) and np.array_equal(npu, onp)
    finally:
        batch.close()
        snap.close()
