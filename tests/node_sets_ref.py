"""Reference values for per-pod candidate node sets, from the CPU oracle's verify matrix (no device).

The oracle itself knows no sets: a pair outside the pod's set fails a Filter before every koord plugin, so the expected
keys are the top-k of make_key(total, i) over the pairs with status 0 whose node is a candidate, and the expected
verify word is the oracle's with KG_ST_NODE_EXCLUDED ORed in. The sequential replay is rebuilt from one verify row per
step on the oracle state's current table, followed by the oracle's Assume."""
import numpy as np

import oracle_lib
from koordinator_amd import abi, nodesets

EXCLUDED = 0x8000  # KG_ST_NODE_EXCLUDED, restated (test_node_sets_host.py checks the header and the package against it)
STATE_KEYS = ("req_cpu", "req_mem", "req_eph", "num_pods", "nz_cpu", "nz_mem", "sc_req0", "sc_req1")

CLUSTERS = {
    "small": lambda synth: synth.small(300, 64),                 # both storage classes
    "mixed": lambda synth: synth.mixed(240, 160, seed=31),       # F_BIG records, integer lanes
    "n33": lambda synth: synth.small(33, 8),                     # a last bitmap word of one bit
    "n129": lambda synth: synth.small(129, 70, seed=3),          # class boundary off the 64-record grid
}


def all_keys(status, total, mask=None):
    """uint64[P, N]: make_key(total, i) where status is 0 (and node i is a candidate), else 0."""
    p, n = status.shape
    node = np.uint64(0xFFFFFFFF) - np.arange(n, dtype=np.uint64)
    keys = ((total.astype(np.int64) & 0xFFFFFFFF).astype(np.uint64) << np.uint64(32)) | node[None, :]
    ok = status == 0
    if mask is not None:
        ok &= np.asarray(mask, bool)
    return np.where(ok, keys, np.uint64(0))


def expected_keys(status, total, mask, k):
    """uint64[P, k]: the descending top-k of all_keys per pod, zero-filled."""
    keys = all_keys(status, total, mask)
    if keys.shape[1] < k:
        keys = np.concatenate([keys, np.zeros((keys.shape[0], k - keys.shape[1]), np.uint64)], axis=1)
    return np.sort(keys, axis=1)[:, ::-1][:, :k].copy()


def expected_status(status, mask):
    """The verify word with sets: the oracle's | KG_ST_NODE_EXCLUDED where the node is no candidate."""
    return np.where(np.asarray(mask, bool), status, status | np.uint32(EXCLUDED)).astype(np.uint32)


def kind_masks(status, total, seed=5, winner=None):
    """The set kinds of the tests, dealt by j % 7 -> (mask bool[P, N], pod_set, bits, kind[P]).
      0 no set   1 every node but the pod's unmasked winner   2 only nodes infeasible for the pod   3 the empty set
      4 exactly the pod's second-best node   5 one random half of the nodes, one shared set   6 an explicit all-true set
    winner (optional): the node kind 1 removes, per pod (the replay's unmasked placement); default the select's."""
    p, n = status.shape
    top2 = expected_keys(status, total, None, 2)
    first = abi.key_node(top2[:, 0]) if winner is None else np.asarray(winner)
    second = abi.key_node(top2[:, 1])
    half = np.random.default_rng(seed).random(n) < 0.5
    kind = np.arange(p) % 7
    mask = np.ones((p, n), bool)
    for j in range(p):
        if kind[j] == 1 and first[j] >= 0:
            mask[j, first[j]] = False
        elif kind[j] == 2:
            mask[j] = status[j] != 0
        elif kind[j] == 3:
            mask[j] = False
        elif kind[j] == 4:
            mask[j] = False
            if second[j] >= 0:
                mask[j, second[j]] = True
        elif kind[j] == 5:
            mask[j] = half
    pod_set, bits = nodesets.from_mask(mask)
    # kind 6 is all-true, which from_mask turns into "no set": give those pods an explicit set of every node
    six = kind == 6
    if six.any():
        pod_set[six] = len(bits)
        bits = np.concatenate([bits, nodesets.pack(np.ones((1, n), bool))], axis=0)
    return mask, pod_set, bits, kind


def step_replay(kc, nodes, pods, mask):
    """One pod per cycle over an OracleState: (node, total, reason, state). Each cycle takes the top-1 key of the pod's
    candidates from a verify row on the state's current table, ORs the expected verify words into reason, and Assumes."""
    p = abi.table_len(pods)
    state = oracle_lib.OracleState(kc, nodes)
    node = np.full(p, -1, np.int32)
    total = np.full(p, -1, np.int64)
    reason = np.zeros(p, np.uint32)
    for j in range(p):
        tbl = dict(nodes)
        tbl.update(state.table())
        ver = oracle_lib.eval_verify(kc, tbl, abi.take(pods, [j]))
        words = expected_status(ver.status, mask[j:j + 1])
        reason[j] = np.bitwise_or.reduce(words[0]) if words.size else 0
        key = expected_keys(ver.status, ver.total, mask[j:j + 1], 1)[0, 0]
        if key == 0:
            continue
        i = int(abi.key_node(key))
        if state.assume(i, pods, j):
            node[j], total[j] = i, int(abi.key_total(key))
        else:  # a failing BestEffort Reserve: the pod stays unscheduled, the zone code names the reason
            reason[j] |= np.uint32((int(ver.numa_zone[0, i]) & 7) << 12)
    return node, total, reason, state
