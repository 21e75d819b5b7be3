"""The owning buffer type of the host runtime (koordinator_amd/csrc/kg_devmem.h), checked on the CPU:
tests/native/devmem_main.cpp is a stand-alone program over the header that defines the four allocation functions over
malloc / free (live-allocation count, "fail the N-th allocation" switch), built with the host compiler under
AddressSanitizer and UBSan and run directly. Its cases: alloc, reserve smaller / equal / larger (pointer and cap() after
each), move construction and move assignment (the target's old buffer is freed), reset twice, a struct of six buffers
allocated in a chain with the 1st, 3rd and 6th allocation failing in turn (nothing live after its destruction: the
kg_snapshot_create case), a two-buffer group whose second reserve fails and whose retry leaves both at the new capacity,
a failed reserve on a non-empty buffer (null pointer, cap() == 0), and no live allocation at exit."""
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


def test_devmem_under_sanitizers(tmp_path):
    exe = tmp_path / "devmem_main"
    subprocess.check_call([host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "native", "devmem_main.cpp"),
                           "-o", str(exe)])
    res = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert res.returncode == 0, res.stdout
    assert "devmem ok" in res.stdout
