"""The Filter edge lattice: nodes tuned so that ONE Filter predicate sits at a chosen offset from its threshold for ONE
pod, every other predicate passing with wide room (test_filter_ref.py pins the oracle on it with filter_ref.py,
test_filter_edges.py every device consumer of the Filter with the oracle).

lattice() -> (cfg, nodes, pods, cells), cells[i] = (Pred, delta, pod index) of node i:
- Pred(name, cap, form): name is the predicate ("nrf_pods", "nrf_cpu", ..., "la_cpu", "la_mem", "amp", "zone_cpu",
  "zone_mem"), cap the capacity the predicate divides or subtracts from, form what else the cell is about (the
  LoadAware profile, a zone shape, a special case such as "over" or "thr0");
- delta: request (or base + estimate) minus headroom (or cut-off): the pair passes up to 0 and fails from +1 on,
  unless the form says otherwise (expected_word gives the pair's whole status word).

Capacities: 1, 100, 101, 1000, 96000, 2^44 - 1 (the last fast-path value), 2^44 (the first F_BIG one), 2^46 and 2^50.
Capacity 0 is there for the NodeResourcesFit resources, the pod count and the LoadAware total (where it switches the
resource off); amplified cpu has no cell at capacity 1 (requested >= cpuset >= 1 amplifies to 2 or more), and a zone
without a capacity is outside what filter_ref restates.

Pods: sizes 1, 999, 1000, 7 * 1024^3 and 123456789, each as a prod pod (cpu, memory, ephemeral storage), a koord-batch
pod (both scalars, ephemeral storage) and a general pod (everything), 26 copies apart in nz_mem only (score-only: no
Filter threshold moves). kg_pods_upload orders the fast pods by wave kind and a select loop is specialised only for a
wave of 64 lanes that are all of one kind, so each kind has 130 distinct rows: a run of 127 lanes or more holds a whole
aligned wave wherever it starts (lane_kinds / whole_waves check it; small_rows is a sub-batch of at most 256 lanes,
the one-launch select's limit, built the same way). Then DaemonSet pods, skipped pods, prod pods without HAS_CPU /
HAS_MEM, one-scalar pods, pods without an estimate, pods that request nothing, and pods whose estimate is past 2^44
(integer lanes)."""
from collections import namedtuple

import numpy as np

import filter_ref
import score_ref
from koordinator_amd import abi, synth

Pred = namedtuple("Pred", "name cap form")

SIZES = (1, 999, 1000, 7 * 1024 ** 3, 123456789)
COPIES = 26
ROOM = 1 << 43  # a capacity with wide room for every pod below, inside the fast path
CAPS = (1, 100, 101, 1000, 96000, (1 << 44) - 1, 1 << 44, 1 << 46, 1 << 50)
BIG_EST = (1 << 44) + 5
PROD, DS, SKIP = abi.KG_POD_PROD, abi.KG_POD_DAEMONSET, abi.KG_POD_NUMA_SKIP
HAS = abi.KG_POD_HAS_CPU | abi.KG_POD_HAS_MEM

# LoadAware float points: at e = (2 thr + 1) t / 200 exact arithmetic gives thr + 0.5 (over the threshold), Go's two
# float64 roundings land just below (not over); e + 1 is over either way
FLOAT_TOTALS = (200, 1000, 32000, 96000, 1000 << 20)
FLOAT_THRS = (14, 28, 56, 57, 100)
FLOAT_E_T1000 = {14: 145, 28: 285, 56: 565, 57: 575, 100: 1005}

NRF_RES = {"nrf_cpu": ("alloc_cpu", "req_cpu", "req_cpu", abi.KG_ST_NRF_CPU),
           "nrf_mem": ("alloc_mem", "req_mem", "req_mem", abi.KG_ST_NRF_MEM),
           "nrf_eph": ("alloc_eph", "req_eph", "req_eph", abi.KG_ST_NRF_EPH),
           "nrf_sc0": ("sc_alloc0", "sc_req0", "sc_req0", abi.KG_ST_NRF_SC0),
           "nrf_sc1": ("sc_alloc1", "sc_req1", "sc_req1", abi.KG_ST_NRF_SC1)}
# the wave kinds (test_wave_kinds.wave_kind: 0 prod, 1 koord-batch, 2 general) whose pods can fail the predicate
REACH = {"nrf_pods": ("prod", "batch", "gen"), "nrf_cpu": ("prod", "gen"), "nrf_mem": ("prod", "gen"),
         "nrf_eph": ("prod", "batch", "gen"), "nrf_sc0": ("batch", "gen"), "nrf_sc1": ("batch", "gen"),
         "la_cpu": ("prod", "batch", "gen"), "la_mem": ("prod", "batch", "gen"), "amp": ("prod", "gen"),
         "zone_cpu": ("prod", "gen"), "zone_mem": ("prod", "gen")}
KIND_ID = {"prod": 0, "batch": 1, "gen": 2}


# ---- pods ---------------------------------------------------------------------------------------------------------

def _pod(kind, x, est=None, nz=0):
    """One pod row of a kind at size x (est: its LoadAware estimate of both resources, default x)."""
    p = {c: 0 for c in abi.POD_I64}
    p["flags"] = 0
    if kind in ("prod", "ds", "nohas", "prod_sc"):
        p.update(req_cpu=x, req_mem=x, req_eph=x, flags=PROD | HAS)
        if kind == "ds":
            p["flags"] |= DS
        if kind == "nohas":
            p["flags"] = PROD
        if kind == "prod_sc":
            p["sc_req0"] = 500
    elif kind in ("batch", "sc0", "sc1"):
        p.update(req_eph=x, sc_req0=x if kind != "sc1" else 0, sc_req1=x if kind != "sc0" else 0)
    elif kind in ("gen", "noeph"):
        p.update(req_cpu=x, req_mem=x, req_eph=x if kind == "gen" else 0, sc_req0=x, sc_req1=x, flags=HAS)
    elif kind == "skip":
        p.update(req_eph=x, flags=SKIP)
    elif kind == "zero":
        p.update(flags=SKIP)
    else:
        raise ValueError(kind)
    e = x if est is None else est
    p.update(la_est0=e, la_est1=e)
    p["nz_cpu"] = p["req_cpu"] if p["req_cpu"] else 100
    p["nz_mem"] = (p["req_mem"] if p["req_mem"] else 200 << 20) + nz
    return p


def pod_table():
    """(pods, index): index[key] = the pod's row; keys (kind, size index, copy) for the three wave kinds, (kind, size
    index) for the other families, ("zero",), (kind + "_e0",) for a pod without an estimate, ("bigest", r)."""
    rows, index = [], {}

    def add(key, p):
        index[key] = len(rows)
        rows.append(p)

    for kind in ("prod", "batch", "gen"):
        for s, x in enumerate(SIZES):
            for t in range(COPIES):
                add((kind, s, t), _pod(kind, x, nz=t))
    for kind in ("ds", "skip", "nohas", "sc0", "sc1", "prod_sc", "noeph"):
        for s, x in enumerate(SIZES):
            add((kind, s), _pod(kind, x))
    add(("zero",), _pod("zero", 0))
    for kind in ("prod", "batch", "gen"):
        add((kind + "_e0",), _pod(kind, 1000, est=0, nz=100))
    for r in range(2):  # an estimate past the fast domain on one resource: the integer lanes
        for kind in ("prod", "gen"):
            p = _pod(kind, 1000, nz=200 + r)
            p[f"la_est{r}"] = BIG_EST
            add(("bigest", kind, r), p)
    t = abi.empty_pods(len(rows))
    for j, p in enumerate(rows):
        for c, v in p.items():
            t[c][j] = v
    return t, index


# ---- nodes --------------------------------------------------------------------------------------------------------

def roomy_node():
    """A node row on which every pod of pod_table() but the ("bigest", ..) ones passes every predicate with room."""
    n = {c: 0 for c in abi.NODE_I64}
    for c in ("alloc_cpu", "alloc_mem", "alloc_eph", "sc_alloc0", "sc_alloc1", "la_alloc0", "la_alloc1"):
        n[c] = ROOM
    n.update(alloc_pods=110, la_thr_usage0=100, la_thr_usage1=100, la_flags=abi.KG_LA_HAS_METRIC,
             numa_policy=abi.KG_NUMA_NONE, numa_zones=2, numa_zone_status=0, cpu_amp_ratio=1.0)
    for z in range(2):
        n[f"zone_cpu{z}"] = n[f"zone_mem{z}"] = ROOM // 2
    return n


def node_table(rows):
    t = abi.empty_nodes(len(rows))
    for i, n in enumerate(rows):
        for c, v in n.items():
            t[c][i] = v
    return t


def set_la(n, r, profile, total, thr, base):
    """Resource r of the node on a LoadAware profile: "usage" (plain thresholds; prod pods read them too, with the
    non-prod base, where the node has no prod thresholds), "prod" or "agg". The bases and thresholds the profile does
    NOT read are decoys that give the other verdict next to the threshold."""
    n[f"la_alloc{r}"] = total
    if profile == "usage":
        n[f"la_thr_usage{r}"] = thr
        n[f"la_fbase_np{r}"] = n[f"la_sbase_np{r}"] = base
        n[f"la_fbase_prod{r}"] = n[f"la_sbase_prod{r}"] = base + 1000  # not read
    elif profile == "prod":
        n["la_flags"] |= abi.KG_LA_PROD_THR
        n[f"la_thr_prod{r}"] = thr
        n[f"la_thr_prod{1 - r}"] = n[f"la_thr_prod{1 - r}"] or 100
        n[f"la_fbase_prod{r}"] = n[f"la_sbase_prod{r}"] = base
    elif profile == "agg":
        n["la_flags"] |= abi.KG_LA_AGG_THR
        n[f"la_thr_agg{r}"] = thr
        n[f"la_thr_agg{1 - r}"] = n[f"la_thr_agg{1 - r}"] or 100
        n[f"la_fbase_np{r}"] = n[f"la_sbase_np{r}"] = base
    else:
        raise ValueError(profile)


def la_node(r, profile, total, thr, delta, est):
    """base + est = cut + delta on resource r."""
    cut = filter_ref.la_cut(total, thr)
    n = roomy_node()
    set_la(n, r, profile, total, thr, cut + delta - est)
    return n


def amp_node(cap, ratio, cs, x, delta):
    """filterAmplifiedCPUs: x = alloc - (requested - cs + Amplify(cs)) + delta; None when requested < cs."""
    extra = score_ref.amplify(cs, ratio) - cs
    q = cap - x + delta - extra
    if q < cs:
        return None
    n = roomy_node()
    n.update(alloc_cpu=cap, req_cpu=q, nz_cpu=q, cpu_amp_ratio=ratio, cpuset_alloc_milli=cs)
    return n


def zone_node(res, cap, form, x, delta):
    """A SingleNUMANode node whose zones leave of `res` ("cpu" / "mem"): only1: x - 1 and x - delta; neither: x - delta
    twice; lack: nothing and x - delta; one: a single zone with x - delta; the other resource has room. cross / cross1:
    see below."""
    avail = {"only1": (x - 1, x - delta), "neither": (x - delta, x - delta), "lack": (0, x - delta),
             "one": (x - delta,), "cross": (0, x), "cross1": (1, x)}[form]
    n = roomy_node()
    n.update(numa_policy=abi.KG_NUMA_SINGLE_NODE, numa_zones=len(avail))
    for z, a in enumerate(avail):
        n[f"zone_{res}{z}"] = cap
        n[f"zone_{res}_used{z}"] = cap - a
    if form in ("cross", "cross1"):
        # zone 1 alone has enough of `res`, zone 0 alone of the other resource, of which zone 1 leaves x - delta: past
        # the threshold only both zones together hold the pod, and whether `res` then has a hint at all turns on
        # zone 0 having nothing (cross) or something (cross1) of it left
        other = "mem" if res == "cpu" else "cpu"
        for z, a in enumerate((x, x - delta)):
            n[f"zone_{other}{z}"] = cap
            n[f"zone_{other}_used{z}"] = cap - a
    return n


# ---- the lattice ----------------------------------------------------------------------------------------------------

def _sizes_upto(limit):
    return [s for s, x in enumerate(SIZES) if x <= limit]


def lattice():
    cfg = synth.bench_profile(numa=True)
    pods, ix = pod_table()
    rows, cells = [], []

    def add(n, name, cap, form, delta, key):
        rows.append(n)
        cells.append((Pred(name, cap, form), delta, ix[key]))

    def pick(name, c, limit):
        """(pod key, size) of the cell: the kind cycles over the kinds that reach the predicate, the size over the
        sizes that fit under the capacity."""
        kinds = REACH[name]
        kind = kinds[c % len(kinds)]
        ss = _sizes_upto(limit)
        s = ss[(c + len(name)) % len(ss)]
        return (kind, s, 0), SIZES[s]

    # NodeResourcesFit: the five resources and the pod count over every capacity class
    for name, (a, u, _, _) in NRF_RES.items():
        for c, cap in enumerate(CAPS):
            for delta in ((0, 1, -1) if c in (3, 5, 7) else (0, 1)):
                key, x = pick(name, c, cap - 1 if delta < 0 else cap)
                n = roomy_node()
                n[a], n[u] = cap, cap - x + delta
                if name in ("nrf_cpu", "nrf_mem"):
                    n["nz" + u[3:]] = n[u]
                add(n, name, cap, "", delta, key)
        # a zero request is never insufficient: headroom 0, over capacity (the pod requests the other resources),
        # capacity 0; one unit fails each
        zero = {"nrf_cpu": ("batch", 2, 0), "nrf_mem": ("batch", 2, 0), "nrf_eph": ("noeph", 2),
                "nrf_sc0": ("prod", 2, 0), "nrf_sc1": ("prod", 2, 0)}[name]
        one = (REACH[name][-1], 0, 0)
        for form, cap, used, key, delta in (("h0", 1000, 1000, zero, 0), ("h0", 1000, 1000, one, 1),
                                            ("over", 1000, 1005, zero, 5), ("cap0", 0, 0, zero, 0),
                                            ("cap0", 0, 0, one, 1)):
            n = roomy_node()
            n[a], n[u] = cap, used
            if name in ("nrf_cpu", "nrf_mem"):
                n["nz" + u[3:]] = used
            add(n, name, cap, form, delta, key)
    for c, cap in enumerate(CAPS):
        for delta in ((0, 1, -1) if c in (3, 5, 7) and cap > 1 else (0, 1)):
            key, _ = pick("nrf_pods", c, 1 << 62)
            n = roomy_node()
            n.update(alloc_pods=cap, num_pods=cap - 1 + delta)
            add(n, "nrf_pods", cap, "", delta, key)
    n = roomy_node()
    n.update(alloc_pods=0, num_pods=0)
    add(n, "nrf_pods", 0, "cap0", 1, ("zero",))

    # LoadAware: both resources over every total; the profile and the threshold cycle
    profiles = ("usage", "prod", "agg", "usage_prodpod")
    thrs = (65, 100, 14, 28, 56, 57, 65, 100, 28)
    for r, name in enumerate(("la_cpu", "la_mem")):
        for c, cap in enumerate(CAPS):
            form = profiles[(c + r) % 4]
            kind = {"usage": ("batch", "gen")[c % 2], "prod": "prod", "agg": ("gen", "batch")[c % 2],
                    "usage_prodpod": "prod"}[form]
            cut = filter_ref.la_cut(cap, thrs[c])
            for delta in ((0, 1, -1) if c in (3, 5, 7) else (0, 1)):
                ss = _sizes_upto(cut + delta)
                key = (kind, ss[(c + r) % len(ss)], 0) if ss else (kind + "_e0",)
                est = int(pods["la_est0"][ix[key]])
                add(la_node(r, form.split("_")[0], cap, thrs[c], delta, est), name, cap, form, delta, key)
        # the node already over its cut-off: a pod without an estimate fails too
        add(la_node(r, "usage", 96000, 65, 5, 0), name, 96000, "usage", 5, ("gen_e0",))
        add(la_node(r, "prod", 96000, 65, 5, 0), name, 96000, "prod", 5, ("prod_e0",))
        # an estimate past 2^44 (the pod's integer lanes) on totals past it
        for cap, forms in ((1 << 46, ("prod", "usage")), (1 << 50, ("usage_prodpod", "agg"))):
            for form in forms:
                kind = "gen" if form in ("usage", "agg") else "prod"
                for delta in (0, 1):
                    add(la_node(r, form.split("_")[0], cap, 65, delta, BIG_EST), name, cap, form, delta,
                        ("bigest", kind, r))
        # one threshold zero / one total zero: that resource is skipped however far over it is, the other decides
        o = 1 - r
        oname = ("la_cpu", "la_mem")[o]
        for form in ("thr0", "total0"):
            for delta in (0, 1):
                n = la_node(o, "usage", 96000, 57, delta, 1000)
                n[f"la_fbase_np{r}"] = n[f"la_sbase_np{r}"] = 10 ** 9
                if form == "thr0":
                    n[f"la_thr_usage{r}"], n[f"la_alloc{r}"] = 0, 1000
                else:
                    n[f"la_thr_usage{r}"], n[f"la_alloc{r}"] = 65, 0
                add(n, oname, 96000, form, delta, ("gen", 2, 0))
    # both resources over at once: the first (cpu) is the one reported
    for form, key in (("both", ("gen", 2, 0)), ("both_agg", ("batch", 2, 0)), ("both_prod", ("prod", 2, 0))):
        prof = {"both": "usage", "both_agg": "agg", "both_prod": "prod"}[form]
        n = la_node(0, prof, 96000, 57, 1, 1000)
        set_la(n, 1, prof, 1000, 28, 2000)
        add(n, "la_cpu", 96000, form, 1, key)
    # pairs the Filter lets through before it looks at the usage: a DaemonSet pod, empty thresholds, no NodeMetric, a
    # nil NodeMetric; an expired NodeMetric is decided by the two arguments
    add(la_node(0, "usage", 96000, 65, 1, 1000), "la_cpu", 96000, "ds", 1, ("ds", 2))
    n = la_node(0, "usage", 96000, 65, 1, 1000)
    n.update(la_thr_usage0=0, la_thr_usage1=0)
    add(n, "la_cpu", 96000, "empty", 1, ("gen", 2, 0))
    for form, flags in (("nometric", 0), ("nil", abi.KG_LA_HAS_METRIC | abi.KG_LA_NM_NIL),
                        ("expired", abi.KG_LA_HAS_METRIC | abi.KG_LA_EXPIRED)):
        for delta in ((0, 1) if form == "expired" else (1,)):
            n = la_node(0, "usage", 96000, 65, delta, 1000)
            n["la_flags"] = flags
            add(n, "la_cpu", 96000, form, delta, ("gen", 2, 0))

    # LoadAware float points: e - 1, e, e + 1 around e = (2 thr + 1) t / 200, split between base and estimate in
    # several ways (the pod's size cycles), over the profiles and both resources
    pi = 0
    for t in FLOAT_TOTALS:
        for thr in FLOAT_THRS:
            e = (2 * thr + 1) * t // 200
            for di, delta in enumerate((-1, 0, 1)):
                k = pi + di
                r, prof = k % 2, ("usage", "prod", "agg")[k % 3]
                kind = {"usage": ("gen", "batch", "prod")[(pi // 3) % 3], "prod": "prod",
                        "agg": ("batch", "gen")[(pi // 2) % 2]}[prof]
                ss = _sizes_upto(e + delta)
                key = (kind, ss[k % len(ss)], 0) if (pi + 2 * di) % 5 else (kind + "_e0",)
                est = int(pods["la_est0"][ix[key]])
                n = roomy_node()
                set_la(n, r, prof, t, thr, e + delta - est)
                form = prof if not (prof == "usage" and kind == "prod") else "usage_prodpod"
                add(n, ("la_cpu", "la_mem")[r], t, f"float:{thr}:{form}", delta, key)
            pi += 1

    # amplified cpu: ratios whose ceil lands on an integer (1.5 x 1000), between two (1.5 x 3 = 4.5) and just past one
    # (float64 1.1 x 1000 = 1100.0000000000002 -> 1101, 1.1 x 10 -> 12)
    for c, cap in enumerate(CAPS):
        ratio = (1.5, 1.1)[c % 2]
        for delta in (0, 1):
            key, x = pick("amp", c, cap)
            for cs in ((1000, 3) if ratio == 1.5 else (1000, 10)):
                n = amp_node(cap, ratio, cs, x, delta)
                if n is not None:
                    add(n, "amp", cap, f"{ratio}x{cs}", delta, key)
                    break
    for delta in (0, 1):
        add(amp_node(96000, 1.5, 3, 1000, delta), "amp", 96000, "1.5x3", delta, ("gen", 2, 0))
        add(amp_node(96000, 1.1, 10, 999, delta), "amp", 96000, "1.1x10", delta, ("prod", 1, 0))
    # requested == cpuset: amplified (requested >= cpuset, plugin.go:490): 151000 - 1.5 x 100000 = 1000
    for delta in (0, 1):
        n = amp_node(151000 - delta, 1.5, 100000, 1000, delta)
        assert n["req_cpu"] == n["cpuset_alloc_milli"]
        add(n, "amp", 151000 - delta, "eq", delta, ("prod", 2, 0))
    # requested < cpuset: not amplified (plugin.go:490), the pod fits exactly; amplified it would not
    n = roomy_node()
    n.update(alloc_cpu=96000, req_cpu=95000, nz_cpu=95000, cpu_amp_ratio=1.5, cpuset_alloc_milli=96000)
    add(n, "amp", 96000, "lt", 0, ("prod", 2, 0))

    # NUMA zones of SingleNUMANode nodes
    for res in ("cpu", "mem"):
        name = "zone_" + res
        for c, cap in enumerate(CAPS):
            for delta in (0, 1):
                key, x = pick(name, c, cap)
                add(zone_node(res, cap, "only1", x, delta), name, cap, "only1", delta, key)
        for c, cap in ((3, 1000), (7, 1 << 46)):
            for form in ("neither", "lack", "one", "cross", "cross1"):
                for delta in (0, 1):
                    key, x = pick(name, c + len(form), cap)
                    if form.startswith("cross"):  # a size that needs both zones (not 1)
                        key = (key[0], 2 if cap == 1000 else 3, 0)
                        x = SIZES[key[1]]
                    add(zone_node(res, cap, form, x, delta), name, cap, form, delta, key)
    return cfg, node_table(rows), pods, cells


# ---- what each cell says --------------------------------------------------------------------------------------------

def pod_request(name, pods, j):
    """What pod j asks of the predicate's resource (the pod count: 1)."""
    if name in NRF_RES:
        return int(pods[NRF_RES[name][2]][j])
    if name == "nrf_pods":
        return 1
    if name in ("la_cpu", "la_mem"):
        return int(pods[f"la_est{('la_cpu', 'la_mem').index(name)}"][j])
    return int(pods["req_cpu" if name in ("amp", "zone_cpu") else "req_mem"][j])


def expected_word(kc, cell, nodes, i, pods):
    """The tuned pair's whole Filter status word, from what the cell says (not from any evaluation)."""
    (name, cap, form), delta, j = cell
    if name in NRF_RES or name == "nrf_pods":
        bit = abi.KG_ST_NRF_PODS if name == "nrf_pods" else NRF_RES[name][3]
        return bit if delta > 0 and pod_request(name, pods, j) > 0 else 0
    if name in ("la_cpu", "la_mem"):
        bit = abi.KG_ST_LA_CPU if name == "la_cpu" else abi.KG_ST_LA_MEM
        form = form.split(":")[-1]
        if form in ("ds", "empty", "nometric", "nil"):
            return 0
        if form == "expired" and kc.la_filter_expired:
            return 0 if kc.la_schedule_expired else abi.KG_ST_LA_EXPIRED
        if form in ("agg", "both_agg"):
            bit |= abi.KG_ST_LA_AGG
        return bit if delta > 0 else 0
    if name == "amp":
        return abi.KG_ST_NUMA_AMP_CPU if delta > 0 else 0
    if name in ("zone_cpu", "zone_mem"):
        if delta <= 0:
            return 0
        # a zone with nothing left of the resource keeps the two-zone hint out too (or there is one zone only):
        # the resource has no hint at all; else only the two-zone hint is left, which SingleNUMANode cannot align
        res = name[5:]
        Z = int(nodes["numa_zones"][i])
        left = [int(nodes[f"zone_{res}{z}"][i]) - int(nodes[f"zone_{res}_used{z}"][i]) for z in range(Z)]
        if Z == 1 or min(left) == 0:
            return abi.KG_ST_NUMA_UNSATISFIED
        return abi.KG_ST_NUMA_ALIGN
    raise ValueError(name)


def cap_class(cell):
    return cell[0].cap


def float_cells(cells):
    """[(node, total, thr, delta)] of the LoadAware float points."""
    return [(i, p.cap, int(p.form.split(":")[1]), d) for i, (p, d, _) in enumerate(cells) if p.form.startswith("float:")]


def lane_kinds(pods, rows=None):
    """The wave kind of every select lane in launch order (kg_pods_upload: the fast pods grouped by kind 0, 1, 2, then
    the integer-path pods, 3), for pairwise distinct rows (one lane each)."""
    from test_wave_kinds import wave_kind
    rows = range(abi.table_len(pods)) if rows is None else rows
    slow = [any(int(pods[c][j]) >= 1 << 44 for c in abi.POD_I64) for j in rows]
    return sorted(3 if sl else wave_kind(pods, j) for j, sl in zip(rows, slow))


def whole_waves(kinds):
    """The kinds that fill some aligned wave of 64 lanes."""
    return {kinds[w] for w in range(0, len(kinds) - 63, 64) if len(set(kinds[w:w + 64])) == 1}


def small_rows(pods, index):
    """At most 256 fast pods with every tuned pod among them: 64 lanes of prod pods, 64 of koord-batch pods (whole
    waves), then the general ones."""
    rows = []
    for kind in ("prod", "batch"):
        keys = [(kind, s, t) for t in range(COPIES) for s in range(len(SIZES))][:63]
        rows += [index[k] for k in keys] + [index[(kind + "_e0",)]]
    rows += [index[("gen", s, t)] for t in range(13) for s in range(len(SIZES))]
    rows += [j for k, j in index.items() if k[0] in ("ds", "skip", "nohas", "sc0", "sc1", "prod_sc", "noeph", "zero", "gen_e0")]
    return np.array(rows, np.int64)


def subsample(cells):
    """The delta 0 and +1 cells of every (predicate, form family) once, and the 25 float points at e: about 60 nodes,
    for the consumers that are run on one-node snapshots."""
    seen, out = set(), []
    for i, (p, d, _) in enumerate(cells):
        if p.form.startswith("float:"):
            if d == 0:
                out.append(i)
            continue
        k = (p.name, p.form if p.name.startswith("zone") else "", d)
        if p.form in ("lack", "cross1"):
            continue
        if d in (0, 1) and k not in seen and p.cap in (96000, 1000, (1 << 44) - 1):
            seen.add(k)
            out.append(i)
    return out
