"""Per-pod host score terms for engine.PodBatch.set_node_scores (kg_pods_set_node_scores).

The Score plugins that stay on the host (NodeAffinity preferred terms, TaintToleration PreferNoSchedule, ImageLocality,
PodTopologySpread, InterPodAffinity) hand their score lists over as rows of snapshot positions: a row is one plugin's
raw score of every node for one kind of pod, with the plugin's normalisation mode and weight. pod_terms[j] names up to
KG_SCORE_TERMS rows of pod j (-1: unused slot). Pods a plugin scores alike share one row: the device keeps one table row
per row and sorts its lanes by their rows.
"""
from __future__ import annotations

import numpy as np

from . import abi

TERMS = abi.KG_SCORE_TERMS
RAW, NORMALIZE, NORMALIZE_REVERSE = abi.KG_SCORE_RAW, abi.KG_SCORE_NORMALIZE, abi.KG_SCORE_NORMALIZE_REVERSE
RAW_MAX = abi.KG_SCORE_RAW_MAX
WEIGHT_MAX = 1 << 20


def value(mode: int, raw, feasible) -> np.ndarray:
    """The value of one term on every node, int64[N]: raw for RAW; for the normalised modes DefaultNormalizeScore(100,
    reverse) against m = the largest raw over the pod's feasible candidates (feasible: bool[N], the nodes whose verify
    status word is 0), in integer division. Only the feasible entries mean anything: selectHost reads no other."""
    raw = np.asarray(raw, np.int64)
    feasible = np.asarray(feasible, bool)
    if mode == RAW:
        return raw.copy()
    if mode not in (NORMALIZE, NORMALIZE_REVERSE):
        raise ValueError(f"unknown mode {mode}")
    m = int(raw[feasible].max()) if feasible.any() else 0
    if m == 0:
        return np.full(raw.shape, 100 if mode == NORMALIZE_REVERSE else 0, np.int64)
    q = 100 * raw // m
    return 100 - q if mode == NORMALIZE_REVERSE else q


def from_terms(terms, n_nodes: int):
    """Per pod a list of at most KG_SCORE_TERMS terms (raw int[N], mode, weight), or None / [] for no term ->
    (pod_terms int32[P, KG_SCORE_TERMS], raw int32[R, N], mode uint32[R], weight uint32[R]). Equal rows (same raw, mode
    and weight) share one row, numbered in order of first appearance; a pod's slots fill from the left, the rest stay -1."""
    n_nodes = int(n_nodes)
    pod_terms = np.full((len(terms), TERMS), -1, np.int32)
    ids: dict = {}
    rows, modes, weights = [], [], []
    for j, lst in enumerate(terms):
        lst = list(lst or ())
        if len(lst) > TERMS:
            raise ValueError(f"pod {j}: {len(lst)} terms, at most {TERMS}")
        for t, (raw, mode, weight) in enumerate(lst):
            raw = np.ascontiguousarray(raw, np.int32).reshape(-1)
            if len(raw) != n_nodes:
                raise ValueError(f"pod {j} term {t}: {len(raw)} scores for {n_nodes} nodes")
            if raw.size and (raw.min() < 0 or raw.max() > RAW_MAX):
                raise ValueError(f"pod {j} term {t}: raw outside [0, {RAW_MAX}]")
            if mode not in (RAW, NORMALIZE, NORMALIZE_REVERSE):
                raise ValueError(f"pod {j} term {t}: unknown mode {mode}")
            if not 0 <= int(weight) <= WEIGHT_MAX:
                raise ValueError(f"pod {j} term {t}: weight outside [0, {WEIGHT_MAX}]")
            key = (raw.tobytes(), int(mode), int(weight))
            rid = ids.get(key)
            if rid is None:
                rid = ids[key] = len(rows)
                rows.append(raw)
                modes.append(int(mode))
                weights.append(int(weight))
            pod_terms[j, t] = rid
    raw = np.stack(rows).astype(np.int32) if rows else np.zeros((0, n_nodes), np.int32)
    return pod_terms, raw, np.array(modes, np.uint32), np.array(weights, np.uint32)
