"""Representative rows of a pod batch (koordinator_amd/csrc/kg_dedup.h), checked on the CPU: tests/native/dedup_main.cpp
is a stand-alone program over the header, built with the host compiler under AddressSanitizer and UBSan and run
directly. Its cases: n = 0 and 1, all rows equal, all distinct, rows differing in exactly one column (each int64 column,
the flags word's KG_POD_* bits, its NUMA-policy bits), every case again with a constant hash (every row collides: rep
must still be exact), a second call with a smaller n into the same buffers, and the reduced lane lists."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_compiler():
    for cxx in (os.environ.get("CXX"), "g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    pytest.fail("no host C++ compiler")


def test_dedup_rows_under_sanitizers(tmp_path):
    exe = tmp_path / "dedup_main"
    subprocess.check_call([host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "native", "dedup_main.cpp"),
                           "-o", str(exe)])
    res = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert res.returncode == 0, res.stdout
    assert "dedup ok" in res.stdout
