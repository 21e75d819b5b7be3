"""Reference values for the node offer slots (kg_eval_offer_slots), from the CPU oracle as it is (no device).

calculateNodeOfferSlot (coscheduling/core/network_topology_solver.go:113-158), per node: the job's pods are filtered
one after another on the node with the earlier ones added, the count stops at the first failure. The oracle knows no
such loop; it is rebuilt from one verify row per pod on a copy of the node table: nodes still alive with status 0 gain a
slot and NodeInfo.AddPodInfo's columns (the pod's seven request columns and one pod), the others keep the word. With
candidate node sets the word is node_sets_ref.expected_status of it.

Two wrong readings of the loop, for the tests to show that their inputs tell them apart: no accumulation at all
(leading_passes of the verify matrix on the table as it stands) and the full Reserve between pods (assume_slots:
OracleState.assume, which also moves the LoadAware bases and the NUMA zones)."""
import numpy as np

import node_sets_ref
import oracle_lib
from koordinator_amd import abi

# the node columns NodeInfo.AddPodInfo moves <- the pod column added (num_pods += 1 beside them)
ADD_COLUMNS = (("req_cpu", "req_cpu"), ("req_mem", "req_mem"), ("req_eph", "req_eph"), ("sc_req0", "sc_req0"),
               ("sc_req1", "sc_req1"), ("nz_cpu", "nz_cpu"), ("nz_mem", "nz_mem"))

CLUSTERS = {
    "small": lambda synth: synth.small(300, 64),                          # both storage classes
    "small_x4": lambda synth: synth.small(300, 64, scale=4.0),            # small counts
    "mixed": lambda synth: synth.mixed(240, 160, seed=31),                # F_BIG records and NUMA reason bits
    "n129": lambda synth: synth.small(129, 70, seed=3, scale=4.0),        # class boundary off the 64-record grid
    "n33": lambda synth: synth.small(33, 8),                              # one partial wave
    "cpuset": lambda synth: synth.cpuset_cluster(200, 64),                # cpuset-binding pods
    "topology": lambda synth: synth.topology(200, 64),                    # Restricted / BestEffort policies
}


def row_lists(n_pods):
    """{name: rows (None = every pod in batch order)} of the parity test."""
    head = np.arange(min(48, n_pods), dtype=np.uint32)
    return {"head": head, "reversed": head[::-1].copy(), "all": None, "copies": np.full(40, 3, np.uint32)}


def _rows(pods, rows):
    return np.arange(abi.table_len(pods), dtype=np.uint32) if rows is None else np.asarray(rows, np.uint32)


def own_table(nodes):
    """A node table whose AddPodInfo columns are copies (the others are shared: nothing writes them)."""
    t = dict(nodes)
    for col, _ in ADD_COLUMNS:
        t[col] = np.array(nodes[col], np.int64)
    t["num_pods"] = np.array(nodes["num_pods"], np.int64)
    return t


def add_pod(tbl, sel, pods, j):
    """NodeInfo.AddPodInfo of pod j on the nodes `sel` (bool[N] or indices) of tbl."""
    for col, pcol in ADD_COLUMNS:
        tbl[col][sel] += int(pods[pcol][j])
    tbl["num_pods"][sel] += 1


def offer_slots(kc, nodes, pods, rows=None, mask=None):
    """(slots uint32[N], status uint32[N]) of the pods `rows` (None: batch order); mask: bool[P, N] candidate nodes."""
    n = abi.table_len(nodes)
    tbl = own_table(nodes)
    slots = np.zeros(n, np.uint32)
    word = np.zeros(n, np.uint32)
    alive = np.ones(n, bool)
    for j in _rows(pods, rows):
        j = int(j)
        if not alive.any():
            break
        st = oracle_lib.eval_verify(kc, tbl, abi.take(pods, [j])).status
        if mask is not None:
            st = node_sets_ref.expected_status(st, mask[j:j + 1])
        st = st[0]
        stop = alive & (st != 0)
        word[stop] = st[stop]
        alive &= st == 0
        slots[alive] += 1
        add_pod(tbl, alive, pods, j)
    return slots, word


def leading_passes(status, rows=None):
    """uint32[N]: per node the number of leading rows of status[rows] (uint32[P, N]) that are 0."""
    st = status if rows is None else status[np.asarray(rows, np.int64)]
    bad = st != 0
    first = np.where(bad.any(axis=0), bad.argmax(axis=0), len(st))
    return first.astype(np.uint32)


def plain_slots(kc, nodes, pods, rows=None):
    """The counts without accumulation: every pod on the table as it stands."""
    return leading_passes(oracle_lib.eval_verify(kc, nodes, pods).status, rows)


def assume_slots(kc, nodes, pods, rows=None):
    """The counts with the oracle's whole Reserve (OracleState.assume) between pods."""
    n = abi.table_len(nodes)
    state = oracle_lib.OracleState(kc, nodes)
    slots = np.zeros(n, np.uint32)
    alive = np.ones(n, bool)
    for j in _rows(pods, rows):
        j = int(j)
        if not alive.any():
            break
        tbl = dict(nodes)
        tbl.update(state.table())
        st = oracle_lib.eval_verify(kc, tbl, abi.take(pods, [j])).status[0]
        alive &= st == 0
        for i in np.flatnonzero(alive):
            if state.assume(int(i), pods, j):
                slots[i] += 1
            else:
                alive[i] = False
    return slots
