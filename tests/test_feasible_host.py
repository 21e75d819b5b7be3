"""Host side of the feasible-node bitmaps (kg_eval_feasible; no device): the agreement of include/koordgpu.h and abi.py
on the new symbol and on KG_ST_UNRESOLVABLE_MASK, nodesets.to_mask as the inverse of nodesets.pack, and the launch
geometry of kg_feasible.h in a stand-alone program."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from koordinator_amd import abi, nodesets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "koordgpu.h")


def header():
    with open(HEADER) as f:
        return f.read()


def define(src, name):
    m = re.search(r"^#define %s\s+(0x[0-9A-Fa-f]+)u?\b" % name, src, re.M)
    assert m, name
    return int(m.group(1), 0)


def test_header_declares_the_call_within_abi_14():
    src = header()
    assert re.search(r"^kg_status kg_eval_feasible\(kg_snap\* snap, kg_pods\* pods, const uint32_t\* rows, uint32_t n_rows, "
                     r"uint32_t fail_mask,", src, re.M)
    assert re.search(r"^#define KG_ABI_VERSION 14\b", src, re.M) and abi.KG_ABI_VERSION == 14


def test_unresolvable_mask_agrees_and_is_the_four_documented_bits():
    src = header()
    mask = define(src, "KG_ST_UNRESOLVABLE_MASK")
    assert mask == abi.KG_ST_UNRESOLVABLE_MASK
    # exactly the KG_ST_* bits whose own comment says UnschedulableAndUnresolvable (a comment may run over two lines)
    said = set()
    for m in re.finditer(r"^#define (KG_ST_\w+)\s+(0x[0-9A-Fa-f]+)u?[ \t]*/\*(.*?)\*/", src, re.M | re.S):
        if "UnschedulableAndUnresolvable" in m.group(3) and not m.group(1).endswith("_MASK"):
            said.add(m.group(1))
    assert said == {"KG_ST_NUMA_CONFLICT", "KG_ST_NUMA_CPU_TOPO", "KG_ST_NUMA_CPU_BIND", "KG_ST_DEV_NO_DEVICE"}
    want = 0
    for name in said:
        assert define(src, name) == getattr(abi, name)
        want |= define(src, name)
    assert mask == want == 0x02620000


def test_unresolvable_mask_is_disjoint_from_the_host_side_bits():
    src = header()
    mask = define(src, "KG_ST_UNRESOLVABLE_MASK")
    for name in ("KG_ST_NODE_EXCLUDED", "KG_ST_QUOTA", "KG_ST_UNSUPPORTED"):
        assert define(src, name) == getattr(abi, name)
        assert not mask & define(src, name), name


@pytest.mark.parametrize("n", [1, 31, 32, 33, 129])
def test_to_mask_inverts_pack(n):
    rng = np.random.default_rng(n)
    m = rng.random((6, n)) < 0.5
    m[0] = False
    m[1] = True
    m[2] = False
    m[2, n - 1] = True  # the last bit alone
    bits = nodesets.pack(m)
    assert bits.shape == (6, (n + 31) // 32) and bits.dtype == np.uint32
    back = nodesets.to_mask(bits, n)
    assert back.dtype == bool and back.shape == m.shape and np.array_equal(back, m)
    assert np.array_equal(nodesets.pack(back), bits)


def test_to_mask_of_no_nodes():
    assert nodesets.to_mask(np.zeros((3, 0), np.uint32), 0).shape == (3, 0)


def test_geometry_under_sanitizers(tmp_path):
    """tests/native/feasible_geom_main.cpp: the chunk geometry of kg_feasible.h (chunk starts on the 64-record grid for
    n in {1, 63, 64, 65, 100000}, one writer per word, every record covered once), a stand-alone program built with
    the host compiler under AddressSanitizer and UBSan and run directly."""
    cxx = next((shutil.which(c) for c in (os.environ.get("CXX"), "g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++")
                if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "feasible_geom_main"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "native", "feasible_geom_main.cpp"),
                           "-o", str(exe)])
    res = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert res.returncode == 0, res.stdout
    assert "feasible geometry ok" in res.stdout
