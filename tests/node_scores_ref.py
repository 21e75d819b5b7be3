"""Reference values for per-pod host score terms, from the CPU oracle's verify matrix (no device).

The oracle knows no terms and does not have to: total' = total + the sum over a pod's terms of weight x value on the
pairs with status 0 whose node is a candidate, where a normalised term's maximum is taken over exactly those pairs.
The expected keys are node_sets_ref.expected_keys of total'. Written with Python integers pair by pair, apart from
koordinator_amd.nodescores.value (test_node_scores_host.py compares the two)."""
import numpy as np

import node_sets_ref as sets_ref
from koordinator_amd import abi, nodescores

RAW, NORM, REV = 0, 1, 2  # KG_SCORE_*, restated (test_node_scores_host.py checks the header and the package against it)
TERMS = 4
RAW_MAX = 1 << 20

CLUSTERS = sets_ref.CLUSTERS


def term_value(mode, raw, m):
    """One term on one feasible candidate: DefaultNormalizeScore(100, reverse) in Go's integer division."""
    if mode == RAW:
        return raw
    if m == 0:
        return 100 if mode == REV else 0
    q = 100 * raw // m
    return 100 - q if mode == REV else q


def totals(status, total, mask, pod_terms, raw, mode, weight, maximum_over_all=False):
    """int64[P, N]: total' on the feasible candidate pairs (status 0 and, with a mask, a candidate), the oracle's total
    elsewhere. maximum_over_all: the wrong reading of the semantics (the maximum over every node), for the tests that
    show a kind tells the two apart."""
    p, n = status.shape
    ok = status == 0
    if mask is not None:
        ok = ok & np.asarray(mask, bool)
    out = total.astype(np.int64).copy()
    for j in range(p):
        cand = np.flatnonzero(ok[j])
        for t in range(TERMS):
            r = int(pod_terms[j, t])
            if r < 0 or len(cand) == 0:
                continue
            row = raw[r]
            m = int(row.max()) if maximum_over_all else int(row[cand].max())
            for i in cand:
                out[j, i] += int(weight[r]) * term_value(int(mode[r]), int(row[i]), m)
    return out


def expected_keys(status, total, mask, k, *terms):
    return sets_ref.expected_keys(status, totals(status, total, mask, *terms), mask, k)


def expected_verify_total(status, total, mask, *terms):
    """kg_eval_verify's total column: total' where the pair is a feasible candidate, -1 on an excluded pair."""
    out = totals(status, total, mask, *terms)
    return out if mask is None else np.where(np.asarray(mask, bool), out, -1)


def kind_terms(status, total, seed=9):
    """The term kinds of the tests, dealt by j % 8 -> (pod_terms, raw, mode, weight, kind[P], first[P], second[P]).
      0 none   1 RAW w1: 100 on the pod's second-best node   2 NORMALIZE w2: 1000 on an infeasible node, 10 on the
      second-best   3 NORMALIZE_REVERSE w3: 0 on every feasible node, 7 on the others   4 NORMALIZE_REVERSE w3: 5
      everywhere, 2 on the second-best, 50 on an infeasible node   5 kinds 1, 2 and 4 plus a RAW row of weight 0
      6 one NORMALIZE row of random raw in 0..1000 shared by the kind plus a per-pod random RAW row in 0..50
      7 RAW w1: (best - second-best total) on the second-best node."""
    p, n = status.shape
    rng = np.random.default_rng(seed)
    top2 = sets_ref.expected_keys(status, total, None, 2)
    first, second = abi.key_node(top2[:, 0]), abi.key_node(top2[:, 1])
    gap = abi.key_total(top2[:, 0]) - abi.key_total(top2[:, 1])
    kind = np.arange(p) % 8
    shared = rng.integers(0, 1001, n).astype(np.int32)
    terms = []
    for j in range(p):
        bad = int(np.flatnonzero(status[j] != 0)[0])
        z = np.zeros(n, np.int32)

        def k1():
            r = z.copy()
            r[second[j]] = 100
            return (r, RAW, 1)

        def k2():
            r = z.copy()
            r[bad], r[second[j]] = 1000, 10
            return (r, NORM, 2)

        def k4():
            r = np.full(n, 5, np.int32)
            r[second[j]], r[bad] = 2, 50
            return (r, REV, 3)

        if kind[j] == 0:
            terms.append(None)
        elif kind[j] == 1:
            terms.append([k1()])
        elif kind[j] == 2:
            terms.append([k2()])
        elif kind[j] == 3:
            terms.append([(np.where(status[j] == 0, 0, 7).astype(np.int32), REV, 3)])
        elif kind[j] == 4:
            terms.append([k4()])
        elif kind[j] == 5:
            terms.append([k1(), k2(), k4(), (rng.integers(0, 1000, n).astype(np.int32), RAW, 0)])
        elif kind[j] == 6:
            terms.append([(shared, NORM, 1), (rng.integers(0, 51, n).astype(np.int32), RAW, 1)])
        else:
            r = z.copy()
            r[second[j]] = int(gap[j])
            terms.append([(r, RAW, 1)])
    pod_terms, raw, mode, weight = nodescores.from_terms(terms, n)
    return pod_terms, raw, mode, weight, kind, first, second
