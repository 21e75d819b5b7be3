"""The CPU oracle against score_ref.py (an independent restatement in Python integers) on the clusters and
configurations test_config_space.py runs on the GPU, and the residue conditions of weighted_boundary.py: every
weighted mean a case claims to exercise has at least 2 % of its scored pairs at residue 0 and at least 2 % at the high
residue (W - 1, or hi_residue() where that is out of reach). All on the CPU; nothing here is marked gpu.

The boundary clusters' pods differ within a variant only in req_eph (not scored), and every variant has the same number
of pods: the checks run on one pod per variant, which gives the same fractions as the whole batch."""
import numpy as np
import pytest

import config_cases as cc
import oracle_lib
import score_ref as sr
import weighted_boundary as wb
from koordinator_amd import abi, synth

WEIGHT_CASES = cc.weight_cases()
MIN_SHARE = 0.02


def check_scores(kc, nodes, pods, rows):
    """eval_verify's per-plugin scores and total against score_ref for the pods `rows` on every node; returns how many
    pairs had their NodeNUMAResource score compared (node level + zone)."""
    sub = abi.take(pods, np.asarray(rows))
    got = oracle_lib.eval_verify(kc, nodes, sub)
    n = abi.table_len(nodes)
    numa_seen = 0
    for j in range(len(rows)):
        for i in range(n):
            at = f"pod {rows[j]} node {i}"
            nrf = sr.nrf_score(kc, nodes, i, sub, j) if kc.plugins & abi.KG_PLUGIN_NRF else 0
            la = sr.la_score(kc, nodes, i, sub, j) if kc.plugins & abi.KG_PLUGIN_LA else 0
            assert int(got.score_nrf[j, i]) == nrf, at
            assert int(got.score_la[j, i]) == la, at
            st = int(got.status[j, i])
            numa = None
            if not kc.plugins & abi.KG_PLUGIN_NUMA:
                numa = 0
            elif not st & (abi.KG_ST_NUMA_MASK | abi.KG_ST_UNSUPPORTED):
                zones = sr.zone_terms(kc, nodes, i, sub, j)
                if zones is not None:
                    z = sr.zone_pick(zones)
                    # (the oracle reports the zone only for a feasible pair: -1 where another plugin's Filter fails)
                    assert z is not None and int(got.numa_zone[j, i]) == (z if st == 0 else -1), at
                    numa = sr.weighted(zones[z][2])
                elif sr.numa_node_level(nodes, i, sub, j):
                    numa = sr.numa_score(kc, nodes, i, sub, j)
            if numa is not None:
                numa_seen += 1
                assert int(got.score_numa[j, i]) == numa, at
                want = -1 if st else int(kc.weight_nrf) * nrf + int(kc.weight_la) * la + int(kc.weight_numa) * numa
                assert int(got.total[j, i]) == want, at
    return numa_seen


def residue_shares(cfg, nodes, pods, mean):
    """(share at residue 0, share at the high residue, pairs scored) of one mean over the pairs its plugin scores:
    no status bit of the plugin under a configuration with only that plugin enabled."""
    kc1 = cc.only(cfg, cc.PLUGIN_OF[mean])
    rows = np.arange(len(wb.VARIANTS))
    sub = abi.take(pods, rows)
    st = oracle_lib.eval_verify(kc1, nodes, sub).status
    lo = hi = scored = 0
    kc = cfg.kg_config()
    for j in range(len(rows)):
        for i in range(abi.table_len(nodes)):
            if st[j, i]:
                continue
            if mean == "nrf":
                means = [sr.nrf_terms(kc, nodes, i, sub, j)]
            elif mean == "la":
                t = sr.la_terms(kc, nodes, i, sub, j)
                means = [t] if t is not None else []
            elif mean == "numa":
                means = [sr.numa_terms(kc, nodes, i, sub, j)] if sr.numa_node_level(nodes, i, sub, j) else []
            else:  # the hint mean of every zone and the score mean of the chosen one
                zones = sr.zone_terms(kc, nodes, i, sub, j)
                means = [h for _, h, _ in zones] + [zones[sr.zone_pick(zones)][2]] if zones is not None else []
            for t in means:
                r = sr.residue(t)
                if r is None:
                    continue
                scored += 1
                W = r[1]
                ws = tuple(w for _, w in t)
                top = wb.hi_residue("la" if mean == "la" else "nrf", la_key(kc) if mean == "la" else ws)
                lo += r[0] == 0
                hi += r[0] == top
    return lo / max(scored, 1), hi / max(scored, 1), scored


def la_key(kc):
    return (int(kc.la_w[0]), int(kc.la_w[1]), int(kc.la_dominant_w))


@pytest.mark.parametrize("name,cfg,means", WEIGHT_CASES, ids=[c[0] for c in WEIGHT_CASES])
def test_boundary_cluster_oracle_and_residues(name, cfg, means):
    nodes, pods, vj, vi = wb.cluster(cfg, seed=31)
    assert np.array_equal(vj[:len(wb.VARIANTS)], np.arange(len(wb.VARIANTS)))
    assert check_scores(cfg.kg_config(), nodes, pods, list(range(len(wb.VARIANTS)))) > 200
    for mean in means:
        lo, hi, scored = residue_shares(cfg, nodes, pods, mean)
        print(f"{name} {mean}: {scored} scored means, residue 0 {lo:.3f}, high residue {hi:.3f}")
        assert scored >= 100 and lo >= MIN_SHARE and hi >= MIN_SHARE, (mean, lo, hi, scored)


SWITCH_CASES = cc.switch_cases() + [("heavy", cc.heavy())]


@pytest.mark.parametrize("name,cfg", SWITCH_CASES, ids=[c[0] for c in SWITCH_CASES])
@pytest.mark.parametrize("mask", [7, 5, 3])
def test_synthetic_clusters_oracle(name, cfg, mask):
    """The plain synthetic clusters of test_config_space.py (sampled: 48 nodes x 24 pods each) under the configurations
    beyond the fast path's weight domain and the heavy one, with plugins masked."""
    kc = cfg.kg_config()
    kc.plugins = mask
    _, nodes, pods = synth.small(48, 24, seed=5, numa=True)
    assert check_scores(kc, nodes, pods, list(range(24))) > (300 if mask & 4 else 0)
    _, nodes, pods = synth.topology(48, 24, seed=2)
    check_scores(kc, nodes, pods, list(range(24)))
