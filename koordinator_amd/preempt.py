"""Host side of the preemption dry run (PostFilter): the resident table kg_eval_preempt removes victims from, and the
choice of one node among its candidates.

build_residents turns the decoded pods of every node into the rows of kg_snapshot_upload_residents: priority
(corev1helpers.PodPriority), start time (util.GetPodStartTime), the preemption group (the quota name as an id), the
KG_RES_* flags and the PodDisruptionBudgets the pod counts against (filterPodsWithPDBViolation's matching,
elasticquota/preempt.go:224-269: same namespace, a non-empty selector that matches, the pod not in DisruptedPods).
The library orders each node's rows by util.MoreImportantPod; importance_order restates that order.

pick_one_node restates upstream's pickOneNodeForPreemption over kg_eval_preempt's per-node summaries. PARITY UNPINNED:
upstream's source is not available to this project and koord's OrderedScoreFuncs returns nil (elasticquota/
preempt.go:285-287), so the default criteria apply; they are restated here from their documentation.
"""
from __future__ import annotations

import datetime
import json
from typing import Callable, Dict, Optional, Sequence, Tuple

import numpy as np

from . import abi, decode
from .config import SchedulerConfig
from .rsvmatch import label_selector_matches

LABEL_QUOTA_PREEMPTIBLE = "quota.scheduling.koordinator.sh/preemptible"     # extension.LabelPreemptible
LABEL_DISABLE_PREEMPTIBLE = "scheduling.koordinator.sh/disable-preemptible"  # extension.LabelDisablePreemptible
LABEL_QUOTA_NAME = "quota.scheduling.koordinator.sh/name"
ANN_RESOURCE_STATUS = "scheduling.koordinator.sh/resource-status"

DEFAULT_QUOTA_NAME = "koordinator-default-quota"  # extension.DefaultQuotaName

ELASTIC_QUOTA, RESERVATION = "elasticquota", "reservation"


def _md(obj) -> dict:
    return obj.get("metadata") or {}


def pod_priority(pod) -> int:
    """corev1helpers.PodPriority: spec.priority, 0 when unset."""
    p = (pod.get("spec") or {}).get("priority")
    return int(p) if p is not None else 0


def parse_time(t) -> int:
    """A metav1.Time (RFC 3339 string, or already a number) as unix seconds."""
    if isinstance(t, (int, float)):
        return int(t)
    d = datetime.datetime.fromisoformat(str(t).replace("Z", "+00:00"))
    if d.tzinfo is None:
        d = d.replace(tzinfo=datetime.timezone.utc)
    return int(d.timestamp())


def pod_start_time(pod, now: int) -> int:
    """util.GetPodStartTime: status.startTime; an assumed or bound pod that has not started yet counts as `now`."""
    t = (pod.get("status") or {}).get("startTime")
    return parse_time(t) if t else int(now)


def is_non_preemptible(pod, plugin: str = ELASTIC_QUOTA) -> bool:
    """elasticquota: extension.IsPodNonPreemptible (label preemptible == "false"); reservation:
    !extension.IsPodPreemptible (label disable-preemptible == "true")."""
    labels = _md(pod).get("labels") or {}
    if plugin == RESERVATION:
        return labels.get(LABEL_DISABLE_PREEMPTIBLE) == "true"
    return labels.get(LABEL_QUOTA_PREEMPTIBLE) == "false"


def has_numa_allocation(pod) -> bool:
    """The pod holds a cpuset or NUMA-zone allocation (the resource-status annotation NodeNUMAResource's PreBind
    writes; nodenumaresource/preempt.go:227-237 getPodAllocated is non-empty for it)."""
    raw = (_md(pod).get("annotations") or {}).get(ANN_RESOURCE_STATUS)
    if not raw:
        return False
    try:
        st = json.loads(raw)
    except ValueError:
        return False
    return bool(st.get("cpuset")) or bool(st.get("numaNodeResources"))


def can_preempt(preemptor_priority: int, preemptor_group: int, victim_priority: int, victim_group: int,
                victim_flags: int, flags: int) -> bool:
    """The potential-victim rule of kg_eval_preempt (step 1), which canPreempt (elasticquota/preempt.go:289-310,
    flags = SKIP_NON_PREEMPTIBLE | SAME_GROUP) and reservation/preemption.go:154-155 (SKIP_NON_PREEMPTIBLE) instantiate."""
    if (flags & abi.KG_PREEMPT_SKIP_NON_PREEMPTIBLE) and (victim_flags & abi.KG_RES_NON_PREEMPTIBLE):
        return False
    if (flags & abi.KG_PREEMPT_SAME_GROUP) and victim_group != preemptor_group:
        return False
    return victim_priority < preemptor_priority


def selector_valid(sel: dict) -> bool:
    """metav1.LabelSelectorAsSelector returns no error: known operators, values with In / NotIn only."""
    for req in sel.get("matchExpressions") or []:
        op, vals = req.get("operator"), req.get("values") or []
        if op in ("In", "NotIn"):
            if not vals:
                return False
        elif op in ("Exists", "DoesNotExist"):
            if vals:
                return False
        else:
            return False
    return True


def matching_pdbs(pod, pdbs: Sequence[dict]) -> list:
    """Indices of the budgets filterPodsWithPDBViolation decrements for this pod."""
    md = _md(pod)
    labels = md.get("labels") or {}
    if not labels:  # a pod with no labels matches no PDB
        return []
    out = []
    for b, pdb in enumerate(pdbs):
        if (_md(pdb).get("namespace") or "") != (md.get("namespace") or ""):
            continue
        sel = (pdb.get("spec") or {}).get("selector")
        # a PDB with a nil or empty selector matches nothing
        if not sel or not (sel.get("matchLabels") or sel.get("matchExpressions")) or not selector_valid(sel):
            continue
        if not label_selector_matches(sel, labels):
            continue
        if md.get("name") in ((pdb.get("status") or {}).get("disruptedPods") or {}):
            continue
        out.append(b)
    return out


def pdb_allowed(pdbs: Sequence[dict]) -> np.ndarray:
    """int32[len(pdbs)]: Status.DisruptionsAllowed of each budget, kg_eval_preempt's pdb_allowed."""
    return np.array([int((p.get("status") or {}).get("disruptionsAllowed") or 0) for p in pdbs], np.int32)


def split_pdb_violation(budgets: Sequence[Sequence[int]], allowed: Sequence[int]) -> Tuple[list, list]:
    """filterPodsWithPDBViolation over pods given by the budget ids each counts against, in order: (violating,
    non-violating) positions, both in the input's order."""
    left = [int(a) for a in allowed]
    viol, ok = [], []
    for k, ids in enumerate(budgets):
        bad = False
        for b in ids:
            left[b] -= 1
            bad |= left[b] < 0
        (viol if bad else ok).append(k)
    return viol, ok


def importance_order(priority, start_time) -> np.ndarray:
    """Positions ordered by util.MoreImportantPod: higher priority first, then earlier start time; ties keep the input
    order (upstream's sort.Slice is not stable there: parity unpinned on ties)."""
    priority = np.asarray(priority, np.int64)
    start_time = np.asarray(start_time, np.int64)
    return np.lexsort((start_time, -priority)).astype(np.int64)  # lexsort is stable


def build_residents(pods_by_node: Sequence[Sequence[dict]], pdbs: Sequence[dict] = (), cfg: Optional[SchedulerConfig] = None,
                    plugin: str = ELASTIC_QUOTA, now: int = 0, group_of: Optional[Callable[[dict], Optional[str]]] = None,
                    groups: Optional[Dict[str, int]] = None,
                    disable_default_quota_preemption: bool = True) -> Tuple[abi.Table, Dict[str, int]]:
    """(resident table, group ids) of pods_by_node[i] = the decoded pods running on the node at snapshot position i.

    pdbs: decoded PodDisruptionBudgets; budget id b of the table is pdbs[b] (pdb_allowed(pdbs) goes to eval_preempt).
    plugin: whose non-preemptible rule sets KG_RES_NON_PREEMPTIBLE. now: the start time of pods without one.
    group_of(pod) -> quota name, the caller's getPodAssociateQuotaName (default: the quota-name label, else the default
    quota; under plugin "reservation" no group); the names are numbered into `groups` (extended in place when given), a
    pod without one gets -1. A preemptor's group is groups.get(its quota name, -1).
    disable_default_quota_preemption (ElasticQuotaArgs, default true; plugin "elasticquota" only): a pod of the default
    quota is no victim (canPreempt, preempt.go:304-307): it is flagged KG_RES_NON_PREEMPTIBLE."""
    cfg = cfg or SchedulerConfig()
    groups = {} if groups is None else groups
    if group_of is None:
        if plugin == RESERVATION:
            group_of = lambda pod: None  # noqa: E731
        else:
            group_of = lambda pod: (_md(pod).get("labels") or {}).get(LABEL_QUOTA_NAME) or DEFAULT_QUOTA_NAME  # noqa: E731
    rows = [(i, pod) for i, pods in enumerate(pods_by_node) for pod in pods]
    t = abi.empty_residents(len(rows))
    for k, (i, pod) in enumerate(rows):
        t["node"][k] = i
        t["priority"][k] = pod_priority(pod)
        t["start_time"][k] = pod_start_time(pod, now)
        name = group_of(pod)
        t["group"][k] = -1 if name is None else groups.setdefault(name, len(groups))
        flags = 0
        if is_non_preemptible(pod, plugin) or (plugin == ELASTIC_QUOTA and disable_default_quota_preemption
                                               and name == DEFAULT_QUOTA_NAME):
            flags |= abi.KG_RES_NON_PREEMPTIBLE
        if has_numa_allocation(pod):
            flags |= abi.KG_RES_NUMA_ALLOC
        ids = matching_pdbs(pod, pdbs)
        if len(ids) > abi.KG_RES_PDBS:
            flags |= abi.KG_RES_PDB_OVERFLOW
        for b, pid in enumerate(ids[:abi.KG_RES_PDBS]):
            t[f"pdb{b}"][k] = pid
        t["flags"][k] = flags
        v = decode.pod_request_vec(pod, cfg)  # NODEINFO_KEYS + sc_req order: what NodeInfo.RemovePod subtracts
        for name_, x in zip(decode.NODEINFO_KEYS, v):
            t[name_][k] = x
        for s in range(abi.KG_NSCALAR):
            t[f"sc_req{s}"][k] = v[len(decode.NODEINFO_KEYS) + s]
    return t, groups


def victim_positions(mask_words) -> np.ndarray:
    """Positions set in one node's victim mask (uint32[KG_PREEMPT_MASK_WORDS])."""
    w = np.asarray(mask_words, np.uint32).reshape(-1)
    bits = (w[:, None] >> np.arange(32, dtype=np.uint32)[None, :]) & 1
    return np.flatnonzero(bits.reshape(-1))


def pick_one_node(summary) -> int:
    """pickOneNodeForPreemption over one preemptor's row of kg_eval_preempt (a record array [n_nodes] of
    abi.PREEMPT_NODE_DTYPE): the node index, or -1 without a candidate. Only KG_PREEMPT_CANDIDATE nodes with
    n_victims > 0 take part (a candidate without victims means the pod fits as it is: no preemption needed). The
    criteria, each narrowing the nodes the one before it left:
      1. fewest PDB violations (n_violating);
      2. lowest highest victim priority (top_priority);
      3. lowest sum of (priority + 2^31) over the victims;
      4. fewest victims;
      5. latest start time of the highest-priority victims' earliest start (top_start);
      6. lowest index.
    PARITY UNPINNED (module docstring)."""
    s = np.asarray(summary)
    idx = np.flatnonzero((s["result"] == abi.KG_PREEMPT_CANDIDATE) & (s["n_victims"] > 0))
    if not len(idx):
        return -1
    n_vic = s["n_victims"][idx].astype(np.int64)
    keys = [
        s["n_violating"][idx].astype(np.int64),
        s["top_priority"][idx].astype(np.int64),
        # Python ints: sum + n * 2^31 stays exact
        np.array([int(a) + int(n) * (1 << 31) for a, n in zip(s["sum_priority"][idx], n_vic)], dtype=object),
        n_vic,
        -s["top_start"][idx].astype(np.int64),
    ]
    for c in range(len(keys)):
        best = min(keys[c])
        keep = np.array([k == best for k in keys[c]], bool)
        idx = idx[keep]
        keys = [k[keep] for k in keys]
        if len(idx) == 1:
            break
    return int(idx[0])
