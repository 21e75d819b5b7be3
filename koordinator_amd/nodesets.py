"""Per-pod candidate node sets for engine.PodBatch.set_node_sets (kg_pods_set_node_sets).

Before koord's plugins run, the scheduler has narrowed each pod's nodes (nodeSelector and required node affinity,
taints and tolerations, spec.nodeName, NodeUnschedulable, PodTopologySpread, a nominated node, a PreFilterResult). The
host hands the result over as sets of snapshot positions: pod_set[j] names pod j's set (-1: every node), bits[set] is
the set's bitmap, bit (i & 31) of word (i >> 5) = the node at row i of the node upload is a candidate. Pods narrowed
alike share one set: the device keeps one table row per set and sorts its lanes by set.
"""
from __future__ import annotations

import numpy as np


def words(n_nodes: int) -> int:
    """uint32 words of one set's bitmap."""
    return (int(n_nodes) + 31) // 32


def pack(mask) -> np.ndarray:
    """bool[S, N] -> uint32[S, words(N)], bit (i & 31) of word (i >> 5) = mask[:, i]; the tail bits are 0."""
    mask = np.asarray(mask, bool)
    if mask.ndim != 2:
        raise ValueError("mask must be [sets, nodes]")
    s, n = mask.shape
    w = words(n)
    padded = np.zeros((s, w * 32), bool)
    padded[:, :n] = mask
    by = np.packbits(padded.reshape(s, w, 4, 8), axis=-1, bitorder="little").reshape(s, w, 4)
    return np.ascontiguousarray(by).view("<u4").reshape(s, w).astype(np.uint32)


def unpack(bits, n_nodes: int) -> np.ndarray:
    """uint32[S, words(N)] -> bool[S, N]."""
    bits = np.ascontiguousarray(bits, "<u4").reshape(-1, words(n_nodes))
    by = bits.view(np.uint8).reshape(len(bits), -1)
    return np.unpackbits(by, axis=1, bitorder="little")[:, :n_nodes].astype(bool)


def to_mask(bits, n_nodes: int) -> np.ndarray:
    """The inverse of pack for the bitmaps that come back from the device (engine.eval_feasible): uint32[R,
    words(N)] -> bool[R, N], [R, 0] for 0 nodes. unpack under the name of the direction it is used in there."""
    n_nodes = int(n_nodes)
    if n_nodes == 0:
        return np.zeros((len(np.asarray(bits)), 0), bool)
    return unpack(bits, n_nodes)


def from_mask(mask):
    """bool[P, N] (mask[j, i]: pod j may use the node at snapshot position i) -> (pod_set int32[P], bits uint32[S,
    words(N)]). Equal rows share one set, numbered in order of first appearance; an all-true row becomes -1."""
    mask = np.asarray(mask, bool)
    if mask.ndim != 2:
        raise ValueError("mask must be [pods, nodes]")
    p, n = mask.shape
    pod_set = np.full(p, -1, np.int32)
    ids: dict = {}
    rows = []
    packed = pack(mask) if p else np.zeros((0, words(n)), np.uint32)
    full = mask.all(axis=1) if p else np.zeros(0, bool)
    for j in range(p):
        if full[j]:
            continue
        key = packed[j].tobytes()
        sid = ids.get(key)
        if sid is None:
            sid = ids[key] = len(rows)
            rows.append(packed[j])
        pod_set[j] = sid
    bits = np.stack(rows).astype(np.uint32) if rows else np.zeros((0, words(n)), np.uint32)
    return pod_set, bits


def from_lists(lists, n_nodes: int):
    """Per pod a list of candidate node indices (snapshot positions), or None for every node -> (pod_set, bits) as
    from_mask gives them. An empty list is the empty set: the pod has no candidate."""
    n_nodes = int(n_nodes)
    mask = np.ones((len(lists), n_nodes), bool)
    for j, nodes in enumerate(lists):
        if nodes is None:
            continue
        idx = np.asarray(list(nodes), np.int64).reshape(-1)
        if idx.size and (idx.min() < 0 or idx.max() >= n_nodes):
            raise ValueError(f"pod {j}: node index outside [0, {n_nodes})")
        mask[j] = False
        mask[j, idx] = True
    return from_mask(mask)
