"""An independent restatement of the Filter status word, in plain Python integers, for checking the CPU oracle.

Written from the reference's Go sources and, for the upstream NodeResourcesFit; not from the
oracle's C nor from the kernels:
- NodeResourcesFit fitsRequest (upstream v1.35.6, SURVEY §8 c-1 "NodeResourcesFit Fits"): "Too many pods" when
  len(Pods) + 1 > AllowedPodNumber; a pod requesting nothing fits; cpu, memory and ephemeral-storage are insufficient
  only for a request above zero and above allocatable - requested; a scalar is checked only when requested (quantity
  not zero) and not ignored (NodeResourcesFitArgs IgnoredResources / IgnoredResourceGroups);
- LoadAware Filter (loadaware/load_aware.go:150-220) with filterNodeUsage (:316-345): the DaemonSet exemption (:156),
  the profile choice (:161-171), empty thresholds (:172), no NodeMetric (:191-197), an expired one (:200-206), a nil
  one (:207-210), then per resource in vector order a zero threshold (:318) or zero total (:322) skipped and
  int64(math.Round(float64(estimated) / float64(total) * 100)) (:326) compared with the threshold, the FIRST resource
  over it reported (:342), under the aggregated reason on the aggregated profile (:331-334);
- NodeNUMAResource Filter (nodenumaresource/plugin.go:363-459), only where score_ref.numa_node_level / zone_terms
  delimit the pair: a skipped pod (:368), filterAmplifiedCPUs (:461-498) on nodes without a NUMA policy, and on
  SingleNUMANode nodes with idle zones FilterByNUMANode (topology_hint.go:31-41) for a pod that requests cpu and
  memory without a policy or cpuset: the hints of resource_manager.go:529-657 through the single-numa-node merge
  (frameworkext/topologymanager/policy_single_numa_node.go:52-90, policy.go:139-181). Every other pair is None.

Tables are the column dicts of koordinator_amd.abi; every value is converted to int before any arithmetic."""
import math

import score_ref
from koordinator_amd import abi

_i = score_ref._i

NRF_BITS = abi.KG_ST_NRF_MASK
LA_BITS = abi.KG_ST_LA_MASK


# ---- NodeResourcesFit ---------------------------------------------------------------------------------------------

def nrf_bits(kc, nodes, i, pods, j) -> int:
    st = 0
    if _i(nodes, "num_pods", i) + 1 > _i(nodes, "alloc_pods", i):
        st |= abi.KG_ST_NRF_PODS
    req = [_i(pods, c, j) for c in ("req_cpu", "req_mem", "req_eph")]
    sc = [_i(pods, f"sc_req{k}", j) for k in range(abi.KG_NSCALAR)]
    if not any(req) and not any(sc):  # "pod request all zero -> fit"
        return st
    for q, a, u, bit in zip(req, ("alloc_cpu", "alloc_mem", "alloc_eph"), ("req_cpu", "req_mem", "req_eph"),
                            (abi.KG_ST_NRF_CPU, abi.KG_ST_NRF_MEM, abi.KG_ST_NRF_EPH)):
        if q > 0 and q > _i(nodes, a, i) - _i(nodes, u, i):
            st |= bit
    for k, q in enumerate(sc):
        if q == 0 or (int(kc.nrf_ignored_scalars) >> k) & 1:
            continue
        if q > _i(nodes, f"sc_alloc{k}", i) - _i(nodes, f"sc_req{k}", i):
            st |= (abi.KG_ST_NRF_SC0, abi.KG_ST_NRF_SC1)[k]
    return st


# ---- LoadAware ----------------------------------------------------------------------------------------------------

def usage_percent(estimated: int, total: int) -> int:
    """int64(math.Round(float64(estimated) / float64(total) * 100)), load_aware.go:326: two float64 operations, each
    rounded, then math.Round (half away from zero; p - floor(p) is exact in float64)."""
    p = (float(estimated) / float(total)) * 100.0
    if p < 0:
        return -usage_percent(-estimated, total)
    r = math.floor(p)
    return int(r) + (1 if p - r >= 0.5 else 0)


def usage_percent_exact(estimated: int, total: int) -> int:
    """The same percentage in exact arithmetic (what the plugin does NOT compute): round half up of 100 e / t."""
    from fractions import Fraction
    return math.floor(Fraction(100 * estimated, total) + Fraction(1, 2))


def la_cut(total: int, thr: int, hi: int = 1 << 62) -> int:
    """The largest estimated >= 0 whose usage_percent is <= thr (-1: none), by bisection over this module's
    usage_percent (monotone in estimated)."""
    if usage_percent(0, total) > thr:
        return -1
    lo = 0
    if usage_percent(hi, total) <= thr:
        return hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if usage_percent(mid, total) <= thr:
            lo = mid
        else:
            hi = mid
    return lo


def la_bits(kc, nodes, i, pods, j) -> int:
    pf = _i(pods, "flags", j)
    if pf & abi.KG_POD_DAEMONSET:  # :156
        return 0
    f = _i(nodes, "la_flags", i)
    prod_pod = bool(f & abi.KG_LA_PROD_THR) and bool(pf & abi.KG_POD_PROD)  # :161
    is_agg = False
    if prod_pod:
        thr = "la_thr_prod"
    elif f & abi.KG_LA_AGG_THR:
        thr, is_agg = "la_thr_agg", True
    else:
        thr = "la_thr_usage"
    if all(_i(nodes, f"{thr}{r}", i) == 0 for r in range(abi.KG_LA_R)):  # :172 usageThresholds.Empty()
        return 0
    if not f & abi.KG_LA_HAS_METRIC:  # :195 NotFound
        return 0
    if kc.la_filter_expired and f & abi.KG_LA_EXPIRED:  # :200-206
        return 0 if kc.la_schedule_expired else abi.KG_ST_LA_EXPIRED
    if f & abi.KG_LA_NM_NIL:  # :207
        return 0
    base = "la_fbase_prod" if prod_pod else "la_fbase_np"  # GetNodeMetricAndEstimatedOfExisting(.., prodPod, ..)
    for r in range(abi.KG_LA_R):
        value = _i(nodes, f"{thr}{r}", i)
        if value == 0:
            continue
        total = _i(nodes, f"la_alloc{r}", i)
        if total == 0:
            continue
        estimated = _i(nodes, f"{base}{r}", i) + _i(pods, f"la_est{r}", j)
        if usage_percent(estimated, total) <= value:
            continue
        return (abi.KG_ST_LA_CPU, abi.KG_ST_LA_MEM)[r] | (abi.KG_ST_LA_AGG if is_agg else 0)
    return 0


# ---- NodeNUMAResource ---------------------------------------------------------------------------------------------

def amp_bits(nodes, i, pods, j) -> int:
    """filterAmplifiedCPUs (plugin.go:461-498) for a pod that binds no cpuset."""
    pod_cpu = _i(pods, "req_cpu", j)
    ratio = float(nodes["cpu_amp_ratio"][i])
    if pod_cpu == 0 or ratio <= 1:
        return 0
    allocated = _i(nodes, "cpuset_alloc_milli", i)
    requested = _i(nodes, "req_cpu", i)
    if requested >= allocated and allocated > 0:
        requested = requested - allocated + score_ref.amplify(allocated, ratio)
    return abi.KG_ST_NUMA_AMP_CPU if pod_cpu > _i(nodes, "alloc_cpu", i) - requested else 0


def _zone_scope(nodes, i, pods, j):
    """score_ref.zone_terms' conditions, for one zone and more: (Z, request (cpu, mem), avail per zone) or None."""
    fl = _i(pods, "flags", j)
    want = abi.KG_POD_HAS_CPU | abi.KG_POD_HAS_MEM
    nb = nodes.get("cpu_bind_policy")
    Z = _i(nodes, "numa_zones", i)
    if (_i(nodes, "numa_policy", i) != abi.KG_NUMA_SINGLE_NODE or _i(pods, "numa_policy", j) != abi.KG_NUMA_NONE
            or fl & (abi.KG_POD_NUMA_SKIP | abi.KG_POD_CPU_BIND) or fl & want != want
            or float(nodes["cpu_amp_ratio"][i]) > 1 or Z < 1 or _i(nodes, "numa_zone_status", i) != 0
            or (nb is not None and int(nb[i]))):
        return None
    req = (_i(pods, "req_cpu", j), _i(pods, "req_mem", j))
    if min(req) <= 0:
        return None
    tot = [(_i(nodes, f"zone_cpu{z}", i), _i(nodes, f"zone_mem{z}", i)) for z in range(Z)]
    used = [(_i(nodes, f"zone_cpu_used{z}", i), _i(nodes, f"zone_mem_used{z}", i)) for z in range(Z)]
    if any(t <= 0 for z in tot for t in z) or any(u < 0 for z in used for u in z):
        return None
    avail = [tuple(max(t - u, 0) for t, u in zip(tz, uz)) for tz, uz in zip(tot, used)]
    return Z, req, avail


def _split_ok(q: int, avail) -> bool:
    """tryBestToDistributeEvenly of one resource over two zones (resource_manager.go:264-318): the zones in ascending
    availability (sort.Slice, :276; for the mask of zones 0 and 1 the positions are the zone ids), each given
    min(available, remaining / zones left) (splitQuantity :320, allocateRes :336); it fails when some is left."""
    order = [0, 1] if not avail[1] < avail[0] else [1, 0]
    for t, z in enumerate(order):
        q -= min(avail[z], q // (2 - t))
    return q == 0


def zone_bits(kc, nodes, i, pods, j):
    """FilterByNUMANode under SingleNUMANode: 0 when some zone holds both requests (its single-zone hints merge to a
    preferred hint); else the provider's hint lists decide: a requested resource without any hint gives
    "Unsatisfied NUMA <resource>" (policy.go:166-173), hints of two zones only are dropped by filterSingleNumaHints and
    the default hint is not preferred ("NUMA Topology affinity ... cannot aligned", policy_single_numa_node.go:85-88).
    None outside the scope (more than two zones without an eligible one included)."""
    sc = _zone_scope(nodes, i, pods, j)
    if sc is None:
        return None
    Z, req, avail = sc
    if Z >= 2:
        zt = score_ref.zone_terms(kc, nodes, i, pods, j)
        if zt is None:
            return None
        elig = [e for e, _, _ in zt]
    else:
        elig = [all(0 < r <= a for r, a in zip(req, avail[0]))]
    if any(elig):
        return 0
    if Z == 1:
        return abi.KG_ST_NUMA_UNSATISFIED
    if Z > 2:
        return None
    # no single zone allocates; the mask of both zones gives each resource a hint when the allocation of BOTH
    # resources succeeds over it (:590-603) and no zone of it lacks the resource (generateHints :636)
    both = all(_split_ok(req[r], [avail[0][r], avail[1][r]]) for r in range(2))
    for r in range(2):
        lack = avail[0][r] == 0 or avail[1][r] == 0
        if not both or lack:
            return abi.KG_ST_NUMA_UNSATISFIED
    return abi.KG_ST_NUMA_ALIGN


def numa_bits(kc, nodes, i, pods, j):
    """The pair's NodeNUMAResource Filter bits, None where this module does not restate the plugin."""
    if _i(pods, "flags", j) & abi.KG_POD_NUMA_SKIP:  # plugin.go:368 state.skip
        return 0
    if score_ref.numa_node_level(nodes, i, pods, j):
        return amp_bits(nodes, i, pods, j)
    return zone_bits(kc, nodes, i, pods, j)


def status(kc, nodes, i, pods, j):
    """(NodeResourcesFit | LoadAware bits of the enabled plugins, NodeNUMAResource bits or None when the plugin is on
    and the pair is outside the restated scope)."""
    st = 0
    if kc.plugins & abi.KG_PLUGIN_NRF:
        st |= nrf_bits(kc, nodes, i, pods, j)
    if kc.plugins & abi.KG_PLUGIN_LA:
        st |= la_bits(kc, nodes, i, pods, j)
    numa = numa_bits(kc, nodes, i, pods, j) if kc.plugins & abi.KG_PLUGIN_NUMA else 0
    return st, numa


def status_word(kc, nodes, i, pods, j):
    """The whole Filter status word, None for a pair outside the scope."""
    st, numa = status(kc, nodes, i, pods, j)
    return None if numa is None else st | numa


def status_matrix(kc, nodes, pods):
    """(word uint32-valued int64[P, N] under NRF | LA bits, numa int64[P, N] with -1 outside the scope)."""
    import numpy as np
    P, N = abi.table_len(pods), abi.table_len(nodes)
    word = np.zeros((P, N), np.int64)
    numa = np.zeros((P, N), np.int64)
    for j in range(P):
        for i in range(N):
            st, nm = status(kc, nodes, i, pods, j)
            word[j, i] = st
            numa[j, i] = -1 if nm is None else nm
    return word, numa
