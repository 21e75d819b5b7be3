"""The oracle's Filter against an independent restatement (filter_ref.py, written from the Go sources), on the edge
lattice of filter_edges.py (every predicate on, one below and one above its threshold) and on ordinary clusters; and
the lattice against itself: every cell's tuned pair has exactly the outcome the cell says, every predicate shows both
outcomes on every capacity class and in every wave kind that reaches it. No device."""
import functools
from fractions import Fraction

import numpy as np
import pytest

import filter_edges
import filter_ref
import oracle_lib
from koordinator_amd import abi, synth
from test_wave_kinds import wave_kind


@functools.lru_cache(maxsize=None)
def lat():
    """(kc, nodes, pods, cells, oracle status uint32[P, N], ref NRF | LA word [P, N], ref NUMA bits (-1: not
    restated) [P, N]) of the lattice, computed once."""
    cfg, nodes, pods, cells = filter_edges.lattice()
    kc = cfg.kg_config()
    want = oracle_lib.eval_verify(kc, nodes, pods).status
    word, numa = filter_ref.status_matrix(kc, nodes, pods)
    return kc, nodes, pods, cells, want, word, numa


def assert_ref_equals_oracle(kc, nodes, pods, want, word, numa, what):
    """NodeResourcesFit and LoadAware bits on every pair, the whole word where the NUMA plugin is restated."""
    low = filter_ref.NRF_BITS | filter_ref.LA_BITS
    bad = np.argwhere((want & low) != word)
    assert not len(bad), (what, len(bad), [(int(j), int(i), hex(int(want[j, i])), hex(int(word[j, i]))) for j, i in bad[:5]])
    scope = numa >= 0
    bad = np.argwhere(scope & (want != (word | np.where(scope, numa, 0))))
    assert not len(bad), (what, len(bad), [(int(j), int(i), hex(int(want[j, i])), hex(int(word[j, i] | numa[j, i])))
                                           for j, i in bad[:5]])
    return scope


def test_lattice_shape():
    kc, nodes, pods, cells, *_ = lat()
    assert abi.table_len(nodes) == len(cells) <= 450
    kinds = np.array([wave_kind(pods, j) for j in range(abi.table_len(pods))])
    rows = {tuple(int(pods[c][j]) for c in abi.POD_I64) + (int(pods["flags"][j]),) for j in range(len(kinds))}
    assert len(rows) == len(kinds)  # pairwise distinct rows: no two pods share a lane
    for k in (0, 1, 2):
        assert (kinds == k).sum() >= 64, k
    # whole waves of each kind in launch order, in the whole batch and in the 256-lane sub-batch of the top-1 tests
    small = filter_edges.small_rows(pods, filter_edges.pod_table()[1])
    assert len(small) <= 256 and len(set(small.tolist())) == len(small)
    assert filter_edges.whole_waves(filter_edges.lane_kinds(pods)) >= {0, 1, 2}
    assert filter_edges.whole_waves(filter_edges.lane_kinds(pods, small)) >= {0, 1, 2}
    assert 3 not in filter_edges.lane_kinds(pods, small)
    tuned = {j for _, _, j in cells if max(int(pods["la_est0"][j]), int(pods["la_est1"][j])) < filter_edges.BIG_EST}
    assert tuned <= set(small.tolist())
    f = pods["flags"]
    assert (f & abi.KG_POD_DAEMONSET).any() and (f & abi.KG_POD_NUMA_SKIP).any()
    assert ((f & abi.KG_POD_PROD != 0) & (f & (abi.KG_POD_HAS_CPU | abi.KG_POD_HAS_MEM) == 0)).any()
    assert ((pods["sc_req0"] != 0) ^ (pods["sc_req1"] != 0)).any()
    assert (pods["la_est0"] >= 1 << 44).any() and (pods["la_est1"] >= 1 << 44).any()


def test_restatement_equals_oracle_on_the_lattice():
    kc, nodes, pods, cells, want, word, numa = lat()
    scope = assert_ref_equals_oracle(kc, nodes, pods, want, word, numa, "lattice")
    assert scope.mean() > 0.7
    zone_nodes = nodes["numa_policy"] == abi.KG_NUMA_SINGLE_NODE
    assert scope[:, zone_nodes].mean() > 0.3 and (numa[:, zone_nodes] > 0).any()


def test_every_cell_has_exactly_its_outcome():
    """The tuned pair of every cell: the single expected bit for a failing cell, 0 for a passing one, from the
    restatement; no cell outside its scope."""
    kc, nodes, pods, cells, want, word, numa = lat()
    for i, cell in enumerate(cells):
        j = cell[2]
        got = filter_ref.status_word(kc, nodes, i, pods, j)
        exp = filter_edges.expected_word(kc, cell, nodes, i, pods)
        assert got is not None, (i, cell)
        assert got == exp, (i, cell, hex(got), hex(exp))
        assert bin(exp).count("1") <= 1 or exp == abi.KG_ST_LA_CPU | abi.KG_ST_LA_AGG or \
            exp == abi.KG_ST_LA_MEM | abi.KG_ST_LA_AGG, (i, cell)
        assert int(want[j, i]) == exp, (i, cell, hex(int(want[j, i])), hex(exp))


def test_every_predicate_shows_both_outcomes():
    """Per predicate: a passing and a failing cell on every capacity class, in every wave kind that reaches it, and for
    LoadAware on every profile. (Amplified cpu cannot be reached at capacity 1: requested >= cpuset >= 1 amplifies to
    2 or more.)"""
    kc, nodes, pods, cells, *_ = lat()
    by_cap, by_kind, by_form = set(), set(), set()
    for i, cell in enumerate(cells):
        (name, cap, form), delta, j = cell
        fails = filter_edges.expected_word(kc, cell, nodes, i, pods) != 0
        by_cap.add((name, cap, fails))
        by_kind.add((name, wave_kind(pods, j), fails))
        by_form.add((name, form.split(":")[-1], fails))
    for name, kinds in filter_edges.REACH.items():
        for cap in filter_edges.CAPS:
            if name == "amp" and cap == 1:
                continue
            for fails in (False, True):
                assert (name, cap, fails) in by_cap, (name, cap, fails)
        for kind in kinds:
            for fails in (False, True):
                assert (name, filter_edges.KIND_ID[kind], fails) in by_kind, (name, kind, fails)
    for name in ("la_cpu", "la_mem"):
        for form in ("usage", "prod", "agg", "usage_prodpod", "thr0", "total0"):
            for fails in (False, True):
                assert (name, form, fails) in by_form, (name, form, fails)
    for name in ("zone_cpu", "zone_mem"):
        for form in ("only1", "neither", "lack", "one", "cross", "cross1"):
            for fails in (False, True):
                assert (name, form, fails) in by_form, (name, form, fails)
    # the special cases are there
    forms = {(n, f.split(":")[-1]) for (n, _, f), _, _ in cells}
    for name in filter_edges.NRF_RES:
        assert {(name, "h0"), (name, "over"), (name, "cap0")} <= forms
    assert {("la_cpu", x) for x in ("both", "both_agg", "ds", "empty", "nometric", "nil", "expired")} <= forms
    assert {("amp", "lt"), ("amp", "eq")} <= forms


def test_loadaware_float_points():
    """At e = (2 thr + 1) t / 200 the exact percentage is thr + 0.5 and rounds up (over the threshold); Go's two
    float64 roundings land just below, so the plugin lets e through and stops e + 1."""
    kc, nodes, pods, cells, want, word, numa = lat()
    L = oracle_lib.lib()
    for t in filter_edges.FLOAT_TOTALS:
        for thr in filter_edges.FLOAT_THRS:
            e = (2 * thr + 1) * t // 200
            assert (2 * thr + 1) * t % 200 == 0
            if t == 1000:
                assert e == filter_edges.FLOAT_E_T1000[thr]
            assert Fraction(100 * e, t) == thr + Fraction(1, 2)
            assert filter_ref.usage_percent_exact(e, t) == thr + 1  # exact arithmetic: over
            assert filter_ref.usage_percent(e - 1, t) <= thr
            assert filter_ref.usage_percent(e, t) == thr, (t, thr)  # Go: not over
            assert filter_ref.usage_percent(e + 1, t) > thr, (t, thr)
            assert filter_ref.la_cut(t, thr) == e
            for x in (e - 1, e, e + 1):
                assert L.kgo_la_usage_percent(x, t) == filter_ref.usage_percent(x, t), (x, t)
    assert L.kgo_la_usage_percent(575, 1000) == 57 and L.kgo_la_usage_percent(576, 1000) == 58
    pts = filter_edges.float_cells(cells)
    assert len(pts) == 75 and len({(t, thr) for _, t, thr, _ in pts}) == 25
    splits = set()
    for i, t, thr, delta in pts:
        (name, _, form), _, j = cells[i]
        bit = (abi.KG_ST_LA_CPU if name == "la_cpu" else abi.KG_ST_LA_MEM) | (abi.KG_ST_LA_AGG if form.endswith(":agg") else 0)
        assert int(want[j, i]) == (bit if delta > 0 else 0), (i, t, thr, delta)
        splits.add((t, int(pods["la_est0"][j])))
    for t in filter_edges.FLOAT_TOTALS:
        assert len({e for tt, e in splits if tt == t}) >= 2, t  # base / estimate split in more than one way


@pytest.mark.parametrize("ignored", [1, 2, 3])
def test_ignored_scalars(ignored):
    kc0, nodes, pods, cells, *_ = lat()
    cfg = synth.bench_profile(numa=True)
    kc = cfg.kg_config()
    kc.nrf_ignored_scalars = ignored
    idx = [i for i, (p, _, _) in enumerate(cells) if p.name in ("nrf_sc0", "nrf_sc1")]
    sub = abi.take(nodes, idx)
    want = oracle_lib.eval_verify(kc, sub, pods).status
    word, numa = filter_ref.status_matrix(kc, sub, pods)
    assert_ref_equals_oracle(kc, sub, pods, want, word, numa, f"ignored {ignored}")
    for k in range(2):
        bit = (abi.KG_ST_NRF_SC0, abi.KG_ST_NRF_SC1)[k]
        assert bool((want & bit).any()) == (not (ignored >> k) & 1)


@pytest.mark.parametrize("filter_expired,schedule_expired", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_expired_node_metrics(filter_expired, schedule_expired):
    kc0, nodes, pods, cells, *_ = lat()
    kc = synth.bench_profile(numa=True).kg_config()
    kc.la_filter_expired, kc.la_schedule_expired = filter_expired, schedule_expired
    idx = [i for i, (p, _, _) in enumerate(cells) if p.form in ("expired", "nil", "nometric", "empty", "ds")]
    sub = abi.take(nodes, idx)
    want = oracle_lib.eval_verify(kc, sub, pods).status
    word, numa = filter_ref.status_matrix(kc, sub, pods)
    assert_ref_equals_oracle(kc, sub, pods, want, word, numa, "expired")
    for t, i in enumerate(idx):
        cell = cells[i]
        assert int(want[cell[2], t]) == filter_edges.expected_word(kc, cell, nodes, i, pods), cell
    assert bool((want & abi.KG_ST_LA_EXPIRED).any()) == (filter_expired == 1 and schedule_expired == 0)


@pytest.mark.parametrize("seed,scale", [(31, 1.0), (32, 12.0)])
def test_restatement_equals_oracle_on_ordinary_clusters(seed, scale):
    cfg, nodes, pods = synth.small(150, 80, seed=seed, numa=True, scale=scale)
    kc = cfg.kg_config()
    want = oracle_lib.eval_verify(kc, nodes, pods).status
    word, numa = filter_ref.status_matrix(kc, nodes, pods)
    scope = assert_ref_equals_oracle(kc, nodes, pods, want, word, numa, f"seed {seed}")
    assert scope.mean() > 0.8 and 0 < (want == 0).mean() < 1
