"""The host arithmetic of the one-pod-block select (koordinator_amd/csrc/kg_small.h), checked on the CPU:
tests/native/small_plan_main.cpp is a stand-alone program over the header, built with the host compiler under
AddressSanitizer and UBSan and run directly. Its cases: the plan pinned from DESIGN.md §4 (config 2's 48 / 24 records,
251 workgroups and 5 copies at 145 lanes, 48 / 36, 223 and 16 at 64 lanes; the wide rule's lengthening out of
(CUs, 2 CUs); at least 8 compute units; chunk lengths in [8, 64]; at most 4,096 chunks; the shape and F_BIG gates; the form
and replica table; KG_SMALL_CHUNKS), the nine switches read per call, the accumulator parity model over a host array
(the layout and shrinking-lane sequences of test_small_acc_results.py with failed launches in between: the parity handed
out is always all zero), and fold_acc with the status rule against a per-lane brute force."""
import os
import subprocess

from test_devmem_host import ROOT, host_compiler


def test_small_plan_under_sanitizers(tmp_path):
    exe = tmp_path / "small_plan_main"
    subprocess.check_call([host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "native", "small_plan_main.cpp"),
                           "-o", str(exe)])
    res = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert res.returncode == 0, res.stdout
    assert "small plan ok" in res.stdout
