"""KG_ST_* status bits -> the reference plugins' Filter failure reasons (the FitError diagnosis).

The device reports one status word per (pod, node) pair (kg_eval_verify) or, for a replayed pod, the OR
of those words over every node in its cycle (kg_replay out_reason). This module turns the bits back into
the reason strings the Go plugins put into their fwktype.Status, so the caller can build the
unschedulable pod's FitError exactly as the framework would:

  NodeResourcesFit   upstream noderesources.Fits reasons ("Too many pods", "Insufficient <resource>")
  LoadAwareScheduling  pkg/scheduler/plugins/loadaware/load_aware.go:48-51
  NodeNUMAResource   pkg/scheduler/plugins/nodenumaresource/plugin.go:54-63,
                     nodenumaresource/topology_hint.go:37, frameworkext/topologymanager/manager.go:32-33
  DeviceShare        deviceshare/device_allocator.go:434, devicehandler_gpu.go:43 ("Insufficient gpu devices")
  Reservation        reservation/plugin.go:60,68,495
  ElasticQuota       elasticquota/plugin.go:281 ("Insufficient quotas, ...")

Bits that stand for a formatted message carry its fixed prefix; the variable part (which resource, the
quota's numbers) is not encoded in a bit and is left as a placeholder in angle brackets.
"""
from __future__ import annotations

from . import abi

DEFAULT_SCALARS = ("kubernetes.io/batch-cpu", "kubernetes.io/batch-memory")


def _nrf_table(scalar_names):
    return (
        (abi.KG_ST_NRF_PODS, "Too many pods"),
        (abi.KG_ST_NRF_CPU, "Insufficient cpu"),
        (abi.KG_ST_NRF_MEM, "Insufficient memory"),
        (abi.KG_ST_NRF_EPH, "Insufficient ephemeral-storage"),
        (abi.KG_ST_NRF_SC0, f"Insufficient {scalar_names[0]}"),
        (abi.KG_ST_NRF_SC1, f"Insufficient {scalar_names[1]}"),
    )


LA_EXPIRED_REASON = "node(s) nodeMetric expired"
LA_RESOURCES = ((abi.KG_ST_LA_CPU, "cpu"), (abi.KG_ST_LA_MEM, "memory"))


def _la_usage_reason(res: str, aggregated: bool) -> str:
    return f"node(s) {res} aggregated usage exceed threshold" if aggregated else f"node(s) {res} usage exceed threshold"


NUMA_TABLE = (
    (abi.KG_ST_NUMA_AMP_CPU, "Insufficient amplified cpu"),
    (abi.KG_ST_NUMA_CONFLICT, "node(s) NUMA Topology policy not match"),
    (abi.KG_ST_NUMA_NO_RES, "node(s) missing NUMA resources"),
    (abi.KG_ST_NUMA_ALIGN, "Unaligned NUMA Hint cause <hints>"),
    (abi.KG_ST_NUMA_UNSATISFIED, "Unsatisfied NUMA <resource>"),
    (abi.KG_ST_NUMA_CPU_TOPO, "node(s) invalid CPU Topology"),
    (abi.KG_ST_NUMA_CPU_BIND, "node(s) cpu bind policy conflicts / SMT alignment / invalid requested cpus"),
    (abi.KG_ST_NUMA_CPUS, "not enough cpus available to satisfy request"),
    # Reserve of a BestEffort node (plugin.go:612-623, resource_manager.go:135,300-309)
    (abi.KG_ST_NUMA_INSUF_CPU, "Insufficient NUMA cpu"),
    (abi.KG_ST_NUMA_INSUF_MEM, "Insufficient NUMA memory"),
    (abi.KG_ST_NUMA_INSUF_NODE, "node(s) Insufficient NUMA Node resources"),
)
DEV_RSV_REASON = "Reservation(s) Insufficient gpu devices"  # makeReasonsByReservation (deviceshare/plugin.go)
RSV_TABLE = (
    (abi.KG_ST_RSV_AFFINITY, "node(s) no reservations match reservation affinity"),
    (abi.KG_ST_RSV_NODE, "Insufficient <resource> by node"),
    (abi.KG_ST_RSV_RESERVATION, "node(s) no reservation(s) to meet the requirements"),
)
QUOTA_REASON = "Insufficient quotas, <quota state>"
# The node is outside the pod's candidate node set (kg_pods_set_node_sets). The Filter that excluded it ran on the host
# (nodeSelector / affinity, taints, spec.nodeName, PodTopologySpread, ...) and owns the wording: pass its text as
# excluded_reason= where the exact FitError matters.
EXCLUDED_REASON = "node(s) excluded from the pod's candidates"
HOST_PATH_REASON = "pair evaluated by the reference plugin on the host"


def plugin_reasons(bits: int, scalar_names=DEFAULT_SCALARS, excluded_reason=None) -> dict:
    """{plugin name: [reason, ...]} of one status word (or an OR of several). excluded_reason: the wording of
    KG_ST_NODE_EXCLUDED, which belongs to the host Filter that narrowed the pod's nodes (default EXCLUDED_REASON)."""
    bits = int(bits)
    out: dict = {}

    def add(plugin, msg):
        out.setdefault(plugin, []).append(msg)

    if bits & abi.KG_ST_NODE_EXCLUDED:  # the host's Filter ran before every koord plugin
        add("(candidate nodes)", excluded_reason or EXCLUDED_REASON)
    for bit, msg in _nrf_table(scalar_names):
        if bits & bit:
            add("NodeResourcesFit", msg)
    if bits & abi.KG_ST_LA_EXPIRED:
        add("LoadAwareScheduling", LA_EXPIRED_REASON)
    for bit, res in LA_RESOURCES:
        if bits & bit:
            add("LoadAwareScheduling", _la_usage_reason(res, bool(bits & abi.KG_ST_LA_AGG)))
    for bit, msg in NUMA_TABLE:
        if bits & bit:
            add("NodeNUMAResource", msg)
    code = abi.dev_code(bits)
    if code:  # GPU allocator reasons (deviceshare/allocator_gpu.go:31-41, device_allocator.go:432)
        add("DeviceShare", DEV_CODE_REASONS.get(code, "Insufficient gpu devices"))
    if bits & abi.KG_ST_DEV_RSV:
        add("DeviceShare", DEV_RSV_REASON)
    for bit, msg in RSV_TABLE:
        if bits & bit:
            add("Reservation", msg)
    if bits & abi.KG_ST_QUOTA:
        add("ElasticQuota", QUOTA_REASON)
    if bits & abi.KG_ST_UNSUPPORTED:
        add("(host path)", HOST_PATH_REASON)
    return out


DEV_CODE_REASONS = {
    abi.KG_DEV_CODE_INSUFFICIENT: "Insufficient gpu devices",
    abi.KG_DEV_CODE_NO_DEVICE: "Insufficient gpu devices",
    abi.KG_DEV_CODE_GPU_DEVICES: "Insufficient GPU Devices",
    abi.KG_DEV_CODE_TOPO_SCOPED: "Insufficient Topology Scoped GPU Devices",
    abi.KG_DEV_CODE_PARTITIONED: "Insufficient Partitioned GPU Devices",
    abi.KG_DEV_CODE_NO_PARTITION: "node(s) missing GPU Partition Table",
    abi.KG_DEV_CODE_PART_COUNT: "node(s) Unsupported number of GPU requests",
    abi.KG_DEV_CODE_NO_TREE: "node(s) missing GPU Device Topology Tree",
    abi.KG_DEV_CODE_MULTI_SHARED: "node(s) Unsupported Multi-Shared GPU",
    abi.KG_DEV_CODE_NUMA_SCOPED: "Insufficient NUMA Scoped Devices",
    abi.KG_DEV_CODE_NO_TEMPLATE: "no matched GPU shared resource template",
}


def reasons(bits: int, scalar_names=DEFAULT_SCALARS, excluded_reason=None) -> list:
    """Flat list of the reasons in plugin filter order."""
    return [m for msgs in plugin_reasons(bits, scalar_names, excluded_reason).values() for m in msgs]


def _slot(bit: int) -> int:
    return int(bit).bit_length() - 1


def reason_counts(counts_row, scalar_names=DEFAULT_SCALARS, excluded_reason=None) -> dict:
    """{reason string: number of nodes} of one row of engine.eval_diagnose (kg_eval_diagnose): the histogram the
    framework's FitError prints. The strings are plugin_reasons'; DeviceShare's come from the code slots
    (KG_DIAG_DEV_CODE0 + code), not from the code's raw bits; bits that map to one string add up; zero counts are
    left out.

    LoadAware's "aggregated" wording is one bit beside the cpu / memory bit of the same node, so the counts tell how
    many nodes carry it but not, when both resources fail somewhere and only some of those nodes aggregate, how they
    split: then the cpu nodes are taken to be the aggregated ones first (exact whenever every failing node, or none, or
    one resource only is involved)."""
    c = [int(v) for v in counts_row]
    if len(c) != abi.KG_DIAG_SLOTS:
        raise ValueError(f"a diagnosis row has {abi.KG_DIAG_SLOTS} counters, got {len(c)}")
    out: dict = {}

    def add(msg, n):
        if n:
            out[msg] = out.get(msg, 0) + n

    add(excluded_reason or EXCLUDED_REASON, c[_slot(abi.KG_ST_NODE_EXCLUDED)])
    for bit, msg in _nrf_table(scalar_names):
        add(msg, c[_slot(bit)])
    add(LA_EXPIRED_REASON, c[_slot(abi.KG_ST_LA_EXPIRED)])
    agg = c[_slot(abi.KG_ST_LA_AGG)]
    for bit, res in LA_RESOURCES:
        n = c[_slot(bit)]
        a = min(n, agg)
        agg -= a
        add(_la_usage_reason(res, True), a)
        add(_la_usage_reason(res, False), n - a)
    for bit, msg in NUMA_TABLE:
        add(msg, c[_slot(bit)])
    for code in range(1, 16):
        add(DEV_CODE_REASONS.get(code, "Insufficient gpu devices"), c[abi.KG_DIAG_DEV_CODE0 + code])
    add(DEV_RSV_REASON, c[_slot(abi.KG_ST_DEV_RSV)])
    for bit, msg in RSV_TABLE:
        add(msg, c[_slot(bit)])
    add(QUOTA_REASON, c[_slot(abi.KG_ST_QUOTA)])
    add(HOST_PATH_REASON, c[_slot(abi.KG_ST_UNSUPPORTED)])
    return out


def fit_error(counts_row, n_nodes: int, scalar_names=DEFAULT_SCALARS, prefilter_msg=None, excluded_reason=None) -> str:
    """The text of upstream's FitError.Error() (k8s.io/kubernetes pkg/scheduler/framework/types.go) for one row of
    first-plugin counts (engine.eval_diagnose(first_plugin=True): the framework records one failing plugin per node):
    "0/<n_nodes> nodes are available: " + the "<count> <reason>" items sorted as strings, joined by ", " + ".";
    with no failing node just "0/<n_nodes> nodes are available:" (coscheduling/core/core_test.go:569). A pod the
    ElasticQuota PreFilter rejected carries the PreFilter message alone (prefilter_msg: the plugin's formatted text,
    default the placeholder of plugin_reasons). n_nodes: all nodes of the cluster (the sum over shards)."""
    head = f"0/{int(n_nodes)} nodes are available:"
    if int(counts_row[_slot(abi.KG_ST_QUOTA)]):
        return f"{head} {prefilter_msg or QUOTA_REASON}."
    items = sorted(f"{n} {msg}" for msg, n in reason_counts(counts_row, scalar_names, excluded_reason).items())
    return f"{head} {', '.join(items)}." if items else head


def loadaware_status(bits: int):
    """LoadAware bits of one pair -> (code, reason) of the Go Status (load_aware.go:150-220)."""
    msgs = plugin_reasons(int(bits) & abi.KG_ST_LA_MASK).get("LoadAwareScheduling")
    return ("Unschedulable", msgs[0]) if msgs else ("Success", None)
