"""Host side of the FitError diagnosis (no device): counts row -> reason histogram -> FitError text, and the
diagnosis constants of koordinator_amd.abi against include/koordgpu.h."""
import os
import re

import numpy as np
import pytest

from koordinator_amd import abi, reasons

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "koordgpu.h")


def header_define(name):
    with open(HEADER) as f:
        m = re.search(rf"^#define {name}\s+(0x[0-9A-Fa-f]+|\d+)u?\b", f.read(), re.M)
    assert m, f"{name} is not defined in include/koordgpu.h"
    return int(m.group(1), 0)


def row(**slots):
    r = np.zeros(abi.KG_DIAG_SLOTS, np.uint32)
    for k, v in slots.items():
        r[int(k[1:])] = v
    return r


def slot(bit):
    return int(bit).bit_length() - 1


def test_fit_error_single_reason():
    # coscheduling/core/network_topology_workflow_test.go:1255
    r = row(**{f"s{slot(abi.KG_ST_NRF_CPU)}": 8})
    assert reasons.reason_counts(r) == {"Insufficient cpu": 8}
    assert reasons.fit_error(r, 8) == "0/8 nodes are available: 8 Insufficient cpu."


def test_fit_error_sorts_items_as_strings():
    r = row(**{f"s{slot(abi.KG_ST_NRF_CPU)}": 8, f"s{slot(abi.KG_ST_LA_CPU)}": 3, f"s{slot(abi.KG_ST_NRF_PODS)}": 12,
               f"s{abi.KG_DIAG_FEASIBLE}": 0})
    # "12 Too many pods" < "3 node(s) ..." < "8 Insufficient cpu": compared as strings, not by count
    assert reasons.fit_error(r, 23) == ("0/23 nodes are available: 12 Too many pods, "
                                        "3 node(s) cpu usage exceed threshold, 8 Insufficient cpu.")


def test_fit_error_without_failing_node():
    # coscheduling/core/core_test.go:569
    assert reasons.fit_error(row(), 0) == "0/0 nodes are available:"
    assert reasons.reason_counts(row(**{f"s{abi.KG_DIAG_FEASIBLE}": 5})) == {}


def test_bits_sharing_a_string_add_up():
    # DeviceShare codes 1 and 2 both read "Insufficient gpu devices"; the counts come from the code slots, the raw
    # code bits (24, 25, 6, 7) are not reasons of their own
    r = row(**{f"s{abi.KG_DIAG_DEV_CODE0 + abi.KG_DEV_CODE_INSUFFICIENT}": 4,
               f"s{abi.KG_DIAG_DEV_CODE0 + abi.KG_DEV_CODE_NO_DEVICE}": 3,
               f"s{abi.KG_DIAG_DEV_CODE0 + abi.KG_DEV_CODE_GPU_DEVICES}": 2,  # code 3 = bits 24 and 25
               "s24": 4 + 2, "s25": 3 + 2})
    assert reasons.reason_counts(r) == {"Insufficient gpu devices": 7, "Insufficient GPU Devices": 2}
    assert reasons.fit_error(r, 9) == "0/9 nodes are available: 2 Insufficient GPU Devices, 7 Insufficient gpu devices."
    # two scalar resources under one name
    r = row(**{f"s{slot(abi.KG_ST_NRF_SC0)}": 1, f"s{slot(abi.KG_ST_NRF_SC1)}": 2})
    assert reasons.reason_counts(r, scalar_names=("x", "x")) == {"Insufficient x": 3}


def test_loadaware_aggregated_wording():
    r = row(**{f"s{slot(abi.KG_ST_LA_CPU)}": 3, f"s{slot(abi.KG_ST_LA_AGG)}": 3, f"s{slot(abi.KG_ST_LA_EXPIRED)}": 1})
    assert reasons.reason_counts(r) == {"node(s) cpu aggregated usage exceed threshold": 3, "node(s) nodeMetric expired": 1}
    r = row(**{f"s{slot(abi.KG_ST_LA_MEM)}": 5, f"s{slot(abi.KG_ST_LA_AGG)}": 2})
    assert reasons.reason_counts(r) == {"node(s) memory aggregated usage exceed threshold": 2,
                                        "node(s) memory usage exceed threshold": 3}


def test_quota_rejection_carries_the_prefilter_message_alone():
    r = row(**{f"s{slot(abi.KG_ST_QUOTA)}": 6})
    assert reasons.fit_error(r, 6, prefilter_msg="Insufficient quotas, quotaName: q") == \
        "0/6 nodes are available: Insufficient quotas, quotaName: q."
    assert reasons.fit_error(r, 6) == f"0/6 nodes are available: {reasons.QUOTA_REASON}."


def test_reason_strings_are_plugin_reasons():
    """Every single-bit reason of a counts row is the string plugin_reasons gives for that bit."""
    for b in range(32):
        bit = 1 << b
        if bit & (abi.KG_ST_DEV_MASK | abi.KG_ST_LA_AGG):
            continue  # the code's raw bits (counted through the code slots) and the wording bit
        want = reasons.reasons(bit)
        got = reasons.reason_counts(row(**{f"s{b}": 2}))
        assert got == {m: 2 for m in want}, hex(bit)
    for code in range(1, 16):
        want = reasons.reasons(abi.dev_status(code))
        assert reasons.reason_counts(row(**{f"s{abi.KG_DIAG_DEV_CODE0 + code}": 1})) == {want[0]: 1}


def test_row_length_is_checked():
    with pytest.raises(ValueError):
        reasons.reason_counts(np.zeros(32, np.uint32))


def test_abi_matches_header():
    assert abi.KG_ABI_VERSION == header_define("KG_ABI_VERSION") == 14
    for name in ("KG_DIAG_SLOTS", "KG_DIAG_DEV_CODE0", "KG_DIAG_FEASIBLE", "KG_DIAG_FIRST_PLUGIN"):
        assert getattr(abi, name) == header_define(name), name
