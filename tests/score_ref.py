"""An independent restatement of three Score functions, in plain Python integers, for checking the CPU oracle.

Written from the reference's Go sources (the files config.py and SURVEY.md cite), not from the oracle's C:
- NodeResourcesFit: resourceAllocationScorer.score with leastRequestedScore / mostRequestedScore per resource
  (noderesourcefitplus/node_resource_fit_plus_utils.go:36-56, :114-139): cpu and memory use NonZeroRequested, a scalar
  its Requested and only when the pod requests it, a resource of allocatable 0 is skipped together with its weight;
- LoadAware: loadAwareSchedulingScorer / leastUsedScore (loadaware/load_aware.go:235-292, :347-376) with
  ResourceWeights, DominantResourceWeight, the prod profile (ScoreAccordingProdUsage) and the disabled score;
- NodeNUMAResource at node level: scoreWithAmplifiedCPUs (nodenumaresource/scoring.go:132-151) over
  least_allocated.go:30-58 / most_allocated.go:30-62, for nodes without a NUMA topology policy or CPU bind policy and
  pods that bind no cpuset.

Tables are the column dicts of koordinator_amd.abi; every value is converted to int before any arithmetic."""
import math

from koordinator_amd import abi

MAX_NODE_SCORE = 100


def least(requested: int, capacity: int) -> int:
    if capacity == 0 or requested > capacity:
        return 0
    return (capacity - requested) * MAX_NODE_SCORE // capacity


def most(requested: int, capacity: int) -> int:
    if capacity == 0:
        return 0
    return min(requested, capacity) * MAX_NODE_SCORE // capacity


def weighted(terms) -> int:
    """Σ score x weight // Σ weight over (score, weight) terms; 0 without weight."""
    wsum = sum(w for _, w in terms)
    return sum(s * w for s, w in terms) // wsum if wsum > 0 else 0


def _i(t, col, x) -> int:
    return int(t[col][x])


def nrf_terms(kc, nodes, i, pods, j):
    """The (per-resource score, weight) terms that count for the pair."""
    rows = [(_i(nodes, "alloc_cpu", i), _i(nodes, "nz_cpu", i) + _i(pods, "nz_cpu", j), int(kc.nrf_w_cpu)),
            (_i(nodes, "alloc_mem", i), _i(nodes, "nz_mem", i) + _i(pods, "nz_mem", j), int(kc.nrf_w_mem))]
    for k in range(abi.KG_NSCALAR):
        q = _i(pods, f"sc_req{k}", j)
        if q != 0:
            rows.append((_i(nodes, f"sc_alloc{k}", i), _i(nodes, f"sc_req{k}", i) + q, int(kc.nrf_w_sc[k])))
        else:
            rows.append((0, 0, int(kc.nrf_w_sc[k])))
    out = []
    for r, (cap, req, w) in enumerate(rows):
        if w == 0 or cap == 0:
            continue
        out.append(((most if (int(kc.nrf_most_allocated) >> r) & 1 else least)(req, cap), w))
    return out


def nrf_score(kc, nodes, i, pods, j) -> int:
    return weighted(nrf_terms(kc, nodes, i, pods, j))


def la_terms(kc, nodes, i, pods, j):
    """None when the plugin scores the node 0 without a mean (score disabled, no / expired / nil NodeMetric)."""
    if not kc.la_score_enabled:
        return None
    f = _i(nodes, "la_flags", i)
    if not f & abi.KG_LA_HAS_METRIC or f & (abi.KG_LA_EXPIRED | abi.KG_LA_NM_NIL):
        return None
    prod = bool(kc.la_score_prod) and bool(_i(pods, "flags", j) & abi.KG_POD_PROD)
    base = "la_sbase_prod" if prod else "la_sbase_np"
    s = [least(_i(nodes, f"{base}{r}", i) + _i(pods, f"la_est{r}", j), _i(nodes, f"la_alloc{r}", i))
         for r in range(abi.KG_LA_R)]
    terms = [(s[r], int(kc.la_w[r])) for r in range(abi.KG_LA_R)]
    dw = int(kc.la_dominant_w)
    if dw != 0:
        terms.append((min([MAX_NODE_SCORE] + s), dw))
    return terms


def la_score(kc, nodes, i, pods, j) -> int:
    t = la_terms(kc, nodes, i, pods, j)
    return weighted(t) if t is not None else 0


def amplify(origin: int, ratio: float) -> int:
    return origin if ratio <= 1 else int(math.ceil(float(origin) * ratio))


def numa_node_level(nodes, i, pods, j) -> bool:
    """The pairs numa_terms restates: no topology policy on either side, no cpuset binding, Score not skipped."""
    fl = _i(pods, "flags", j)
    nb = nodes.get("cpu_bind_policy")
    return (_i(nodes, "numa_policy", i) == abi.KG_NUMA_NONE and _i(pods, "numa_policy", j) == abi.KG_NUMA_NONE
            and not fl & (abi.KG_POD_NUMA_SKIP | abi.KG_POD_CPU_BIND) and (nb is None or int(nb[i]) == 0))


def numa_terms(kc, nodes, i, pods, j):
    ratio = float(nodes["cpu_amp_ratio"][i])
    pod_cpu = _i(pods, "req_cpu", j)
    req_cpu = _i(nodes, "req_cpu", i)
    if pod_cpu != 0 and ratio > 1:
        held = _i(nodes, "cpuset_alloc_milli", i)
        req_cpu = req_cpu - held + amplify(held, ratio)
    fn = most if kc.numa_most_allocated else least
    out = []
    for cap, req, w in ((_i(nodes, "alloc_cpu", i), req_cpu + pod_cpu, int(kc.numa_w_cpu)),
                        (_i(nodes, "alloc_mem", i), _i(nodes, "req_mem", i) + _i(pods, "req_mem", j), int(kc.numa_w_mem))):
        if cap != 0 and w != 0:
            out.append((fn(req, cap), w))
    return out


def numa_score(kc, nodes, i, pods, j) -> int:
    return weighted(numa_terms(kc, nodes, i, pods, j))


def residue(terms):
    """(Σ s w mod Σ w, Σ w) of a mean's terms; None without weight."""
    W = sum(w for _, w in terms)
    return (sum(s * w for s, w in terms) % W, W) if W > 0 else None


def zone_terms(kc, nodes, i, pods, j):
    """SingleNUMANode node with idle zones, a pod requesting cpu and memory without a policy or cpuset of its own:
    per zone (eligible, hint terms, score terms) as the hint providers and the Score see the zone (requested = total -
    available, nodenumaresource/resource_manager.go GetTopologyHints, scoring.go:168-197). None for any other pair."""
    fl = _i(pods, "flags", j)
    want = abi.KG_POD_HAS_CPU | abi.KG_POD_HAS_MEM
    nb = nodes.get("cpu_bind_policy")
    if (_i(nodes, "numa_policy", i) != abi.KG_NUMA_SINGLE_NODE or _i(pods, "numa_policy", j) != abi.KG_NUMA_NONE
            or fl & (abi.KG_POD_NUMA_SKIP | abi.KG_POD_CPU_BIND) or fl & want != want or float(nodes["cpu_amp_ratio"][i]) > 1
            or _i(nodes, "numa_zones", i) < 2 or _i(nodes, "numa_zone_status", i) != 0 or (nb is not None and int(nb[i]))):
        return None
    req = (_i(pods, "req_cpu", j), _i(pods, "req_mem", j))
    out = []
    for z in range(_i(nodes, "numa_zones", i)):
        tot = (_i(nodes, f"zone_cpu{z}", i), _i(nodes, f"zone_mem{z}", i))
        used = (_i(nodes, f"zone_cpu_used{z}", i), _i(nodes, f"zone_mem_used{z}", i))
        avail = tuple(max(t - u, 0) for t, u in zip(tot, used))
        elig = all(0 < r <= a for r, a in zip(req, avail))
        hint, score = [], []
        for r, (hw, sw) in enumerate(((int(kc.numa_hint_w_cpu), int(kc.numa_w_cpu)), (int(kc.numa_hint_w_mem), int(kc.numa_w_mem)))):
            if tot[r] == 0:
                continue
            if hw:
                hint.append(((most if kc.numa_hint_most_allocated else least)(tot[r] - avail[r] + req[r], tot[r]), hw))
            if sw:
                score.append(((most if kc.numa_most_allocated else least)(used[r] + req[r], tot[r]), sw))
        out.append((elig, hint, score))
    return out


def zone_pick(zones):
    """The zone of the best hint: the highest hint score among the eligible zones, the lowest zone on a tie; None
    when no zone is eligible (the Filter fails)."""
    best = None
    for z, (elig, hint, _) in enumerate(zones):
        if elig and (best is None or weighted(hint) > weighted(zones[best][1])):
            best = z
    return best
