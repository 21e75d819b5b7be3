"""Host side of the per-pod candidate node sets (no device): the reference helpers of node_sets_ref against the CPU
oracle with every node a candidate, koordinator_amd.nodesets' packing, the reason strings of the new status bit, and
the agreement of include/koordgpu.h, abi.py and reasons.py on it."""
import os
import re

import numpy as np
import pytest

import node_sets_ref as ref
import oracle_lib
from koordinator_amd import abi, nodesets, reasons, synth

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "koordgpu.h")


@pytest.mark.parametrize("name", list(ref.CLUSTERS))
@pytest.mark.parametrize("k", [1, 3])
def test_key_helper_equals_the_oracle_select_with_all_true_sets(name, k):
    cfg, nodes, pods = ref.CLUSTERS[name](synth)
    kc = cfg.kg_config()
    ver = oracle_lib.eval_verify(kc, nodes, pods)
    mask = np.ones(ver.status.shape, bool)
    assert np.array_equal(ref.expected_keys(ver.status, ver.total, mask, k), oracle_lib.select(kc, nodes, pods, k))
    # the clusters exercise both outcomes for every pod, and an infeasible pair's total is -1
    assert (ver.status == 0).any(axis=1).all() and (ver.status != 0).any(axis=1).all()
    assert (ver.total[ver.status != 0] == -1).all()


def test_from_mask_shares_sets_and_drops_all_true_rows():
    rng = np.random.default_rng(1)
    a, b = rng.random(70) < 0.5, rng.random(70) < 0.2
    mask = np.stack([a, np.ones(70, bool), b, a, np.zeros(70, bool), b, a])
    pod_set, bits = nodesets.from_mask(mask)
    assert pod_set.dtype == np.int32 and bits.dtype == np.uint32
    assert list(pod_set) == [0, -1, 1, 0, 2, 1, 0]
    assert bits.shape == (3, 3)
    assert np.array_equal(nodesets.unpack(bits, 70), np.stack([a, b, np.zeros(70, bool)]))
    # nothing to narrow: no sets at all
    pod_set, bits = nodesets.from_mask(np.ones((4, 70), bool))
    assert list(pod_set) == [-1] * 4 and bits.shape == (0, 3)


@pytest.mark.parametrize("n", [33, 129])
def test_bit_packing(n):
    rng = np.random.default_rng(n)
    mask = rng.random((5, n)) < 0.5
    mask[0] = False
    mask[0, n - 1] = True  # the single bit of the last word
    mask[1] = False
    mask[1, [0, 31, 32]] = True
    bits = nodesets.pack(mask)
    assert bits.shape == (5, (n + 31) // 32)
    for s in range(5):
        for i in range(n):
            assert bool((int(bits[s, i >> 5]) >> (i & 31)) & 1) == bool(mask[s, i]), (s, i)
    assert int(bits[0, -1]) == 1 and not bits[0, :-1].any()
    assert int(bits[1, 0]) == (1 | 1 << 31) and int(bits[1, 1]) == 1
    tail = (1 << (n & 31)) - 1
    assert not (bits[:, -1] & np.uint32(~tail & 0xFFFFFFFF)).any(), "bits at or above n_nodes are clear"


def test_from_lists():
    pod_set, bits = nodesets.from_lists([[1, 40], None, [], [40, 1], list(range(50))], 50)
    assert list(pod_set) == [0, -1, 1, 0, -1]
    want = np.zeros((2, 50), bool)
    want[0, [1, 40]] = True
    assert np.array_equal(nodesets.unpack(bits, 50), want)
    with pytest.raises(ValueError):
        nodesets.from_lists([[50]], 50)


def test_reason_strings_of_the_excluded_bit():
    bit = abi.KG_ST_NODE_EXCLUDED
    assert reasons.reasons(bit) == ["node(s) excluded from the pod's candidates"]
    assert reasons.reasons(bit, excluded_reason="node(s) didn't match Pod's node affinity/selector") == \
        ["node(s) didn't match Pod's node affinity/selector"]
    # the host's Filter ran first: its reason leads the koord plugins'
    assert reasons.reasons(bit | abi.KG_ST_NRF_CPU) == ["node(s) excluded from the pod's candidates", "Insufficient cpu"]
    row = np.zeros(abi.KG_DIAG_SLOTS, np.uint32)
    row[15], row[1] = 7, 2
    assert reasons.reason_counts(row) == {"node(s) excluded from the pod's candidates": 7, "Insufficient cpu": 2}
    assert reasons.reason_counts(row, excluded_reason="node(s) had untolerated taint") == \
        {"node(s) had untolerated taint": 7, "Insufficient cpu": 2}
    assert reasons.fit_error(row, 9, excluded_reason="node(s) had untolerated taint") == \
        "0/9 nodes are available: 2 Insufficient cpu, 7 node(s) had untolerated taint."


def test_header_abi_and_reasons_agree_on_the_bit():
    with open(HEADER) as f:
        src = f.read()
    m = re.search(r"^#define KG_ST_NODE_EXCLUDED\s+(0x[0-9A-Fa-f]+)u?\b", src, re.M)
    assert m and int(m.group(1), 0) == abi.KG_ST_NODE_EXCLUDED == ref.EXCLUDED == 1 << 15
    masks = [int(x, 0) for x in re.findall(r"^#define KG_ST_\w+_MASK\s+(0x[0-9A-Fa-f]+)u?\b", src, re.M)]
    assert len(masks) >= 5 and not any(v & abi.KG_ST_NODE_EXCLUDED for v in masks), "outside every *_MASK"
    assert "kg_pods_set_node_sets" in src and re.search(r"^#define KG_ABI_VERSION 14\b", src, re.M)
    assert reasons.plugin_reasons(abi.KG_ST_NODE_EXCLUDED) == {"(candidate nodes)": [reasons.EXCLUDED_REASON]}


def test_step_replay_helper_equals_the_oracle_replay_with_all_true_sets():
    cfg, nodes, pods = synth.small(120, 40, scale=4.0)
    kc = cfg.kg_config()
    node, total, reason, state = ref.step_replay(kc, nodes, pods, np.ones((40, 120), bool))
    want_state = oracle_lib.OracleState(kc, nodes)
    wn, wt, wr = want_state.replay(pods, reasons=True)
    assert np.array_equal(node, wn) and np.array_equal(total, wt) and np.array_equal(reason, wr)
    assert (node >= 0).all() and len(set(node.tolist())) == 20
    a, b = state.table(), want_state.table()
    for key in ref.STATE_KEYS:
        assert np.array_equal(a[key], b[key]), key


def test_dedup_with_sets_under_sanitizers(tmp_path):
    """tests/native/dedup_sets_main.cpp: kg_dedup.h with the set id in the row and the split lane lists, a stand-alone
    program built with the host compiler under AddressSanitizer and UBSan and run directly."""
    import shutil
    import subprocess
    root = os.path.dirname(HEADER.rsplit(os.sep, 1)[0])
    cxx = next((shutil.which(c) for c in (os.environ.get("CXX"), "g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++")
                if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "dedup_sets_main"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(root, "tests", "native", "dedup_sets_main.cpp"),
                           "-o", str(exe)])
    res = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert res.returncode == 0, res.stdout
    assert "dedup sets ok" in res.stdout
