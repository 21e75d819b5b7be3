"""Whole-job placement on the device: the FindOneNodePlugin slot driving the replay kernel.

Reference behaviour mirrored here (names, argument meaning, status codes and messages):

  FindOneNodePlugin.FindOneNode, BatchScheduleResult   frameworkext/interface.go:115-145
  how the framework consumes a plan                    frameworkext/framework_extender.go:356-407
  a planner over the whole gang                        coscheduling/core/network_topology_workflow.go:70-160
  BatchScheduler.BatchSchedule                         batch/batch_scheduler.go:74-185
  Engine.RunSchedulingCycle, ValidateAndGroupByRequest batch/engine.go:92-294,348-371
  JobResult.ExampleMessage                             batch/framework/types.go:275-341
  the network-topology planner (PlacePods)             coscheduling/core/network_topology_solver.go:53-418

`ReplayPlanner.find_one_node` places every pending member of the job with the sequential replay kernel
(one pod per cycle, Reserve applied on the device between pods) on the live snapshot and rolls the snapshot
back afterwards (kg_snapshot_checkpoint / kg_snapshot_rollback), so a plan costs no copy of the cluster.
`TopologyPlanner.find_one_node` plans a gang with a network-topology requirement as the reference does: the
per-node offer slots come from the device in one call (kg_eval_offer_slots), `place_pods` then sums them up the
topology tree, picks the lowest topology node under the must-gather layer that holds the job and deals the pods out.
`BatchScheduler.batch_schedule` then runs the inline batch cycle of the plan on the device
(kg_batch_schedule): per planned node, in pod-name order, PreFilter + Filter on that node and Reserve; on any
failure every assumed pod is undone (CleanupAssumedPods) and the job status carries the reference's
example message. Go is not in this image, so this Python layer stands where the Go plugin would; the
numbers all come from the HIP kernels behind include/koordgpu.h (no CPU fallback).
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import abi, engine, reasons

# fwktype.Code values the path returns
SUCCESS = "Success"
ERROR = "Error"
UNSCHEDULABLE = "Unschedulable"
UNSCHEDULABLE_AND_UNRESOLVABLE = "UnschedulableAndUnresolvable"
SKIP = "Skip"

# batch/engine.go:55-68, batch_scheduler.go:96-101, network_topology_workflow.go:37-38
ERR_PRE_FILTER_FAILED = "pre-filter failed for pod {ns}/{name}/{uid}, {msg}"
ERR_FILTER_POD_FAILED = "filter pod {ns}/{name}/{uid} on node {node} failed, err: {msg}"
ERR_RESERVE_POD_FAILED = "reserve pod {ns}/{name}/{uid} on node {node} failed, err: {msg}"
ERR_PLAN_MISSING_NODE = "batch schedule plan missing node for pod {key}"
ERR_NO_PENDING_PODS = "no pending pods"
JOB_SCHEDULE_FAILED = "job batch schedule failed"
# network_topology.go:35 AnnotationGangPodNetworkTopologyIndex
ANNOTATION_TOPOLOGY_INDEX = "gang.scheduling.koordinator.sh/network-topology-index"

# Filter plugin order of the shipped profile: the first failing plugin's reasons make the Status message
_FILTER_ORDER = ("NodeResourcesFit", "LoadAwareScheduling", "NodeNUMAResource", "DeviceShare", "Reservation",
                 "(host path)")


@dataclass
class Status:
    code: str = SUCCESS
    message: str = ""

    def is_success(self) -> bool:
        return self.code == SUCCESS


@dataclass
class JobPod:
    """A member pod as the planner sees it: its key parts and its row of the pod columns (abi.Table)."""
    namespace: str
    name: str
    uid: str = ""
    annotations: Dict[str, str] = field(default_factory=dict)

    @property
    def key(self) -> str:  # batch/framework/types.go:343-345 GetPodKey
        return f"{self.namespace}/{self.name}"


@dataclass
class BatchScheduleResult:
    """frameworkext.BatchScheduleResult: every member pod and its planned node."""
    pods: List[JobPod]
    pod_to_node_name: Dict[str, str]


def topology_index(p: JobPod) -> int:
    """apis/extension/network_topology.go:72-85 GetPodNetworkTopologyIndex (-1 when absent or malformed)."""
    s = p.annotations.get(ANNOTATION_TOPOLOGY_INDEX)
    if s is None:
        return -1
    try:
        return int(s)
    except ValueError:
        return -1


def sort_pods_by_index(idx: Sequence[int], pods: Sequence[JobPod]) -> List[int]:
    """apis/extension/network_topology.go:89-103 SortPodsByIndex: indexed pods first, by index, then by name."""
    def key(i):
        t = topology_index(pods[i])
        return (0, t, pods[i].name) if t >= 0 else (1, 0, pods[i].name)
    return sorted(idx, key=key)


def filter_message(bits: int, scalar_names=reasons.DEFAULT_SCALARS) -> str:
    """The Status message of the first failing Filter plugin (the framework stops at the first failure)."""
    by = reasons.plugin_reasons(bits, scalar_names)
    for plugin in _FILTER_ORDER:
        if plugin in by:
            return ", ".join(by[plugin])
    return ""


class ReplayPlanner:
    """FindOneNodePlugin backed by kg_replay: the whole job is placed on the device in one call."""

    name = "KoordGPUReplayPlanner"

    def __init__(self, snap: engine.Snapshot, node_names: Sequence[str]):
        self.snap = snap
        self.node_names = list(node_names)

    def find_one_node(self, members: Sequence[JobPod], table: abi.Table
                      ) -> Tuple[Optional[BatchScheduleResult], Status, Optional[np.ndarray]]:
        """Plan for all pending members (rows of `table` in `members` order). Returns (plan, status, reason
        bits per member in plan order); Skip when there is no job, Unschedulable when some member finds no
        node (the whole gang must fit: the status names the first such pod and its plugin reasons)."""
        if len(members) == 0:
            return None, Status(SKIP), None
        order = sort_pods_by_index(range(len(members)), members)
        sub = abi.take(table, np.asarray(order, np.int64))
        pods = engine.PodBatch(self.snap.ctx, sub)
        try:
            self.snap.checkpoint()
            try:
                node, _total, why = engine.replay(self.snap, pods, reasons=True)
            finally:
                self.snap.rollback()
        finally:
            pods.close()
        ordered = [members[i] for i in order]
        for t, p in enumerate(ordered):
            if node[t] < 0:
                msg = filter_message(int(why[t])) or "no feasible node"
                return None, Status(UNSCHEDULABLE, f"pod {p.key}: {msg}"), why
        plan = BatchScheduleResult(ordered, {p.key: self.node_names[node[t] - self.snap.index_base]
                                             for t, p in enumerate(ordered)})
        return plan, Status(SUCCESS), why


# ---- the network-topology planner: node offer slots on the device, the topology solver on the host ----------------------
# A restatement of coscheduling/core/network_topology_solver.go:53-111 (PlacePods) and :187-418. The reference keeps a
# TreeNode's children in a Go map and sorts wherever the order matters; here children are walked in name order, so the
# result does not depend on the order they were inserted in.

NODE_TOPOLOGY_LAYER = "NodeTopologyLayer"  # apis/scheduling/v1alpha1/cluster_network_topology_types.go:29
# network_topology_solver.go:22 MessageNoCandidateTopologyNodes
MESSAGE_NO_CANDIDATE_TOPOLOGY_NODES = ("no candidate topology nodes can accommodate job, desiredOfferSlot: {slot}, "
                                       "{nodes}, {fit}")
# the framework stops at a node's first failing plugin: the groups of KG_DIAG_FIRST_PLUGIN (include/koordgpu.h)
_FIRST_PLUGIN_GROUPS = (abi.KG_ST_QUOTA, abi.KG_ST_NODE_EXCLUDED, abi.KG_ST_NRF_MASK, abi.KG_ST_LA_MASK,
                        abi.KG_ST_NUMA_MASK | abi.KG_ST_UNSUPPORTED, abi.KG_ST_DEV_MASK | abi.KG_ST_DEV_RSV,
                        abi.KG_ST_RSV_MASK)


@dataclass(eq=False)
class TopologyNode:
    """networktopology.TreeNode (frameworkext/networktopology/tree.go:93-106). The leaves are NODE_TOPOLOGY_LAYER nodes
    named by node name."""
    layer: str
    name: str
    parent: Optional["TopologyNode"] = None
    children: Dict[str, "TopologyNode"] = field(default_factory=dict)
    offer_slot: int = 0
    score: int = 0
    existing_pod_num: int = 0

    def add_child(self, child: "TopologyNode") -> "TopologyNode":
        child.parent = self
        self.children[child.name] = child
        return child

    def sorted_children(self) -> List["TopologyNode"]:
        return [self.children[k] for k in sorted(self.children) if self.children[k] is not None]


@dataclass
class JobTopologyRequirements:
    """coscheduling/core/network_topology_types.go:33-40."""
    must_gather_layer: str = ""
    desired_offer_slot: int = 0
    layer_pod_count_multiple: Dict[str, int] = field(default_factory=dict)


def copy_topology(root: TopologyNode, parent: Optional[TopologyNode] = None) -> TopologyNode:
    """The tree's shape with every offer slot, score and existing pod count at zero (what place_pods evaluates on)."""
    node = TopologyNode(root.layer, root.name, parent)
    for child in root.sorted_children():
        node.children[child.name] = copy_topology(child, node)
    return node


def enumerate_node_topology_nodes(root: TopologyNode) -> Dict[str, TopologyNode]:
    """network_topology_solver.go:187-210 enumerateNodeTopologyNode: node name -> its leaf."""
    leaves: Dict[str, TopologyNode] = {}
    layer = [root]
    while layer:
        nxt: List[TopologyNode] = []
        for node in layer:
            if node.layer == NODE_TOPOLOGY_LAYER:
                leaves[node.name] = node
            else:
                nxt.extend(node.sorted_children())
        layer = nxt
    return leaves


def evaluate_topology_node(leaves: Dict[str, TopologyNode], node_offer_slot, node_to_score=None,
                           existing_pod_num=None) -> None:
    """network_topology_solver.go:212-233 evaluateTopologyNode: every node's numbers are added to its leaf and to each
    ancestor. A node without a leaf in the tree is left out."""
    node_to_score = node_to_score or {}
    for name, slot in node_offer_slot.items():
        node = leaves.get(name)
        while node is not None:
            node.offer_slot += int(slot)
            node.score += int(node_to_score.get(name, 0))
            node = node.parent
    for name, num in (existing_pod_num or {}).items():
        node = leaves.get(name)
        while node is not None:
            node.existing_pod_num += int(num)
            node = node.parent


def constrain_offer_slot_by_pod_count_multiple(root: TopologyNode, layer_pod_count_multiple) -> None:
    """network_topology_solver.go:239-270: bottom-up, a node's offer slot becomes the sum of its children's constrained
    slots, rounded down to its layer's multiple."""
    if not layer_pod_count_multiple:
        return

    def walk(node: TopologyNode) -> None:
        if node.layer != NODE_TOPOLOGY_LAYER:
            for child in node.sorted_children():
                walk(child)
            node.offer_slot = sum(child.offer_slot for child in node.sorted_children())
        multiple = layer_pod_count_multiple.get(node.layer, 0)
        if multiple > 1:
            node.offer_slot = node.offer_slot // multiple * multiple

    walk(root)


def search_must_gather_satisfied_nodes(requirements: JobTopologyRequirements, root: TopologyNode) -> List[TopologyNode]:
    """network_topology_solver.go:272-301: the topology nodes of the must-gather layer (the root without one)."""
    if not requirements.must_gather_layer:
        return [root]
    found: List[TopologyNode] = []
    layer = [root]
    while not found and layer:
        nxt: List[TopologyNode] = []
        for node in layer:
            if node.layer == requirements.must_gather_layer:
                found.append(node)
            else:
                nxt.extend(node.sorted_children())
        layer = nxt
    return found


def search_offer_slot_satisfied_nodes(requirements: JobTopologyRequirements,
                                      must_gathered: Sequence[TopologyNode]) -> List[TopologyNode]:
    """network_topology_solver.go:303-332: the lowest layer below the must-gather nodes that still has a topology node
    holding the job; its holding nodes."""
    candidates: List[TopologyNode] = []
    layer = list(must_gathered)
    while layer:
        nxt: List[TopologyNode] = []
        holding = [node for node in layer if node.offer_slot >= requirements.desired_offer_slot]
        for node in holding:
            nxt.extend(node.sorted_children())
        if holding:
            candidates = holding
        layer = nxt
    return candidates


def topology_node_less(a: TopologyNode, b: TopologyNode, lower_offer_slot: bool) -> bool:
    """network_topology_solver.go:334-351 topologyNodeLessFunc: more existing pods first, layer by layer upwards; then
    the offer slots layer by layer (fewer first when lower_offer_slot); then the higher score; then the name."""
    x, y = a, b
    while x is not None and y is not None:
        if x.existing_pod_num != y.existing_pod_num:
            return x.existing_pod_num > y.existing_pod_num
        x, y = x.parent, y.parent
    x, y = a, b
    while x is not None and y is not None:
        if x.offer_slot != y.offer_slot:
            return (x.offer_slot < y.offer_slot) == lower_offer_slot
        x, y = x.parent, y.parent
    if a.score != b.score:
        return a.score > b.score
    return a.name < b.name


def sort_topology_nodes(nodes: Sequence[TopologyNode], lower_offer_slot: bool) -> List[TopologyNode]:
    def cmp(a, b):
        return -1 if topology_node_less(a, b, lower_offer_slot) else (1 if topology_node_less(b, a, lower_offer_slot) else 0)
    return sorted(nodes, key=functools.cmp_to_key(cmp))


def distribute_offer_slot(desired_offer_slot: int, node: TopologyNode, distribution: Dict[str, int],
                          layer_pod_count_multiple=None) -> Tuple[List[str], int]:
    """network_topology_solver.go:353-393 distributeOfferSlot: (node names in topology order, slots dealt). Children are
    served largest first, each layer's share rounded down to its multiple."""
    multiples = layer_pod_count_multiple or {}
    max_slot = min(node.offer_slot, desired_offer_slot)
    multiple = multiples.get(node.layer, 0)
    if multiple > 1:
        max_slot = max_slot // multiple * multiple
    if node.layer == NODE_TOPOLOGY_LAYER:
        distribution[node.name] = max_slot
        return [node.name], max_slot
    ordered: List[str] = []
    dealt, remaining = 0, max_slot
    for child in sort_topology_nodes(node.sorted_children(), False):
        names, got = distribute_offer_slot(remaining, child, distribution, multiples)
        ordered.extend(names)
        remaining -= got
        dealt += got
    return ordered, dealt


def distribute_pods(pods: Sequence[JobPod], ordered_nodes: Sequence[str], node_to_offer_slot: Dict[str, int]
                    ) -> Dict[str, str]:
    """network_topology_solver.go:395-418 distributePods: the pods by name over the nodes in topology order."""
    left = dict(node_to_offer_slot)
    pod_to_node: Dict[str, str] = {}
    at = 0
    for p in sorted(pods, key=lambda q: q.name):
        while at < len(ordered_nodes) and left.get(ordered_nodes[at], 0) <= 0:
            at += 1
        if at == len(ordered_nodes):
            raise ValueError(f"{len(pods)} pods over {sum(max(v, 0) for v in node_to_offer_slot.values())} dealt slots")
        pod_to_node[p.key] = ordered_nodes[at]
        left[ordered_nodes[at]] -= 1
    return pod_to_node


def first_plugin_word(word: int) -> int:
    """A status word masked to its first non-empty plugin group (KG_DIAG_FIRST_PLUGIN's order)."""
    for group in _FIRST_PLUGIN_GROUPS:
        if word & group:
            return word & group
    return 0


def first_plugin_counts(words) -> np.ndarray:
    """The row of first-plugin reason counts (engine.eval_diagnose's format, reasons.fit_error's input) of the given
    nodes' status words; zero words count as feasible."""
    row = np.zeros(abi.KG_DIAG_SLOTS, np.uint32)
    for w in words:
        w = first_plugin_word(int(w))
        if w == 0:
            row[abi.KG_DIAG_FEASIBLE] += 1
            continue
        for b in range(32):
            if (w >> b) & 1:
                row[b] += 1
        if w & abi.KG_ST_DEV_MASK:
            row[abi.KG_DIAG_DEV_CODE0 + abi.dev_code(w)] += 1
    return row


def place_pods(root: TopologyNode, node_offer_slot, requirements: JobTopologyRequirements, pods: Sequence[JobPod],
               existing_pod_num=None, node_to_score=None, node_status=None, num_all_nodes: Optional[int] = None
               ) -> Tuple[Optional[Dict[str, str]], str]:
    """network_topology_solver.go:53-111 PlacePods after its first step: node_offer_slot {node name: count} (the
    device's, kg_eval_offer_slots) summed up the tree, the lowest topology node under the must-gather layer that holds
    desired_offer_slot pods, the pods dealt out over its nodes. -> ({pod key: node name}, "") or (None, the reference's
    MessageNoCandidateTopologyNodes text). node_status {node name: status word of the first pod that failed there}
    makes the FitError part of the message, over num_all_nodes nodes (default: the nodes given). Works on its own copy
    of the tree: a pure function of its arguments."""
    tree = copy_topology(root)
    evaluate_topology_node(enumerate_node_topology_nodes(tree), node_offer_slot, node_to_score, existing_pod_num)
    constrain_offer_slot_by_pod_count_multiple(tree, requirements.layer_pod_count_multiple)
    must_gathered = search_must_gather_satisfied_nodes(requirements, tree)
    candidates = search_offer_slot_satisfied_nodes(requirements, must_gathered)
    for candidate in sort_topology_nodes(candidates, True):
        distribution: Dict[str, int] = {}
        ordered, actual = distribute_offer_slot(requirements.desired_offer_slot, candidate, distribution,
                                                requirements.layer_pod_count_multiple)
        if actual >= requirements.desired_offer_slot:
            return distribute_pods(pods, ordered, distribution), ""
    listed = sorted(f"topology topologyNode {n.layer}/{n.name}: {n.offer_slot}" for n in must_gathered)
    words = [w for w in (node_status or {}).values() if int(w)]
    n_all = len(node_offer_slot) if num_all_nodes is None else int(num_all_nodes)
    msg = MESSAGE_NO_CANDIDATE_TOPOLOGY_NODES.format(slot=requirements.desired_offer_slot, nodes=";".join(listed),
                                                     fit=reasons.fit_error(first_plugin_counts(words), n_all))
    if requirements.layer_pod_count_multiple:
        msg += "; podCountMultiple constraints: " + ", ".join(
            sorted(f"{layer}={m}" for layer, m in requirements.layer_pod_count_multiple.items()))
    return None, msg


class TopologyPlanner:
    """FindOneNodePlugin for a gang with a network-topology requirement (network_topology_workflow.go:70-160): the
    per-node offer slots come from the device in one call (kg_eval_offer_slots), the topology solver runs on the host
    (place_pods). Plain snapshots only; a node whose count stopped on KG_ST_UNSUPPORTED offers a lower bound."""

    name = "KoordGPUTopologyPlanner"

    def __init__(self, snap: engine.Snapshot, node_names: Sequence[str], root: TopologyNode):
        self.snap = snap
        self.node_names = list(node_names)
        self.root = root

    def find_one_node(self, members: Sequence[JobPod], table: abi.Table, requirements: JobTopologyRequirements,
                      existing_pod_num=None, node_to_score=None
                      ) -> Tuple[Optional[BatchScheduleResult], Status, Optional[np.ndarray]]:
        """Plan for all pending members (rows of `table` in `members` order) -> (plan, status, offer slots per node of
        the snapshot). Skip when there is no job, Unschedulable with the solver's message when no topology node under
        the must-gather layer holds the job."""
        if len(members) == 0:
            return None, Status(SKIP), None
        order = sort_pods_by_index(range(len(members)), members)
        pods = engine.PodBatch(self.snap.ctx, abi.take(table, np.asarray(order, np.int64)))
        try:
            slots, words = engine.eval_offer_slots(self.snap, pods, status=True)
        finally:
            pods.close()
        ordered = [members[i] for i in order]
        offer = {name: int(slots[i]) for i, name in enumerate(self.node_names)}
        stopped = {name: int(words[i]) for i, name in enumerate(self.node_names) if words[i]}
        pod_to_node, msg = place_pods(self.root, offer, requirements, ordered, existing_pod_num, node_to_score,
                                      node_status=stopped, num_all_nodes=len(self.node_names))
        if pod_to_node is None:
            return None, Status(UNSCHEDULABLE, msg), slots
        return BatchScheduleResult(ordered, pod_to_node), Status(SUCCESS), slots


@dataclass
class JobOutcome:
    status: Status
    pod_status: Dict[str, Status]
    assumed: Dict[str, Tuple[str, int, int]]  # key -> (node, NUMA zone, GPU minors) of the committed pods


class BatchScheduler:
    """batch.BatchScheduler over kg_batch_schedule (the scheduling cycle runs on the device)."""

    def __init__(self, snap: engine.Snapshot, node_names: Sequence[str]):
        self.snap = snap
        self.node_index = {n: i for i, n in enumerate(node_names)}

    def batch_schedule(self, plan: BatchScheduleResult, table_by_key: Dict[str, Tuple[abi.Table, int]]) -> JobOutcome:
        """table_by_key[key] = (pod table, row). Success commits every member's Reserve on the snapshot."""
        for p in plan.pods:
            if not plan.pod_to_node_name.get(p.key):
                return JobOutcome(Status(ERROR, ERR_PLAN_MISSING_NODE.format(key=p.key)), {}, {})
        # buildJobRequest + ValidateAndGroupByRequest: per node, pods by name; nodes in first-appearance order
        groups: Dict[str, List[JobPod]] = {}
        for p in plan.pods:
            groups.setdefault(plan.pod_to_node_name[p.key], []).append(p)
        if not groups:
            return JobOutcome(Status(ERROR, "no pods to schedule"), {}, {})
        batch: List[Tuple[str, JobPod]] = []
        for node_name, ps in groups.items():
            for p in sorted(ps, key=lambda q: q.name):
                batch.append((node_name, p))
        rows = [abi.take(table_by_key[p.key][0], np.asarray([table_by_key[p.key][1]], np.int64)) for _, p in batch]
        sub = abi.concat(rows)
        plan_node = np.asarray([self.node_index[n] - self.snap.index_base for n, _ in batch], np.int32)
        pods = engine.PodBatch(self.snap.ctx, sub)
        try:
            res, stat, zone, minors = engine.batch_schedule(self.snap, pods, plan_node)
        finally:
            pods.close()
        pod_status: Dict[str, Status] = {}
        assumed: Dict[str, Tuple[str, int, int]] = {}
        n_assumed, failed = 0, []
        node_msg: Dict[str, Tuple[int, str]] = {}  # the failing pod's status, set on it and every later pod of its node
        for t, (node_name, p) in enumerate(batch):
            r = int(res[t])
            if r in (abi.KG_BATCH_ASSUMED, abi.KG_BATCH_ROLLED_BACK):
                n_assumed += 1
                pod_status[p.key] = Status(SUCCESS)
                if r == abi.KG_BATCH_ASSUMED:
                    assumed[p.key] = (node_name, int(zone[t]), int(minors[t]))
            elif r in (abi.KG_BATCH_FAILED, abi.KG_BATCH_SIBLING):
                bits = int(stat[t])
                code = UNSCHEDULABLE
                if r == abi.KG_BATCH_SIBLING and node_name in node_msg:
                    # engine.go:188-219: errMsg is formatted once, from the pod that failed, and set on
                    # every pod k >= j of the node group
                    code, msg = node_msg[node_name]
                elif bits & abi.KG_ST_NUMA_RESERVE:
                    code = ERROR  # fwktype.Error (engine.go:278-280)  # Filter passed, the NodeNUMAResource Reserve failed (engine.go:275-283)
                    msg = ERR_RESERVE_POD_FAILED.format(ns=p.namespace, name=p.name, uid=p.uid, node=node_name,
                                                       msg=", ".join(reasons.plugin_reasons(bits & abi.KG_ST_NUMA_RESERVE)
                                                                     ["NodeNUMAResource"]))
                elif bits & abi.KG_ST_QUOTA:  # the ElasticQuota gate runs in PreFilter
                    msg = ERR_PRE_FILTER_FAILED.format(ns=p.namespace, name=p.name, uid=p.uid,
                                                      msg=reasons.plugin_reasons(bits)["ElasticQuota"][0])
                else:
                    msg = ERR_FILTER_POD_FAILED.format(ns=p.namespace, name=p.name, uid=p.uid, node=node_name,
                                                      msg=filter_message(bits))
                if r == abi.KG_BATCH_FAILED:
                    node_msg[node_name] = (code, msg)
                pod_status[p.key] = Status(code, msg)
                failed.append((p.key, node_name))
        if not failed:
            return JobOutcome(Status(SUCCESS), pod_status, assumed)
        # JobResult.ExampleMessage, taken before the cleanup rewrites the assumed pods' statuses
        first_key, first_node = min(failed)
        msg = (f"job failed due to {JOB_SCHEDULE_FAILED}, assumed {n_assumed} pods, failed {len(failed)} pods, "
               f"first failed pod {first_key}@{first_node} failed due to {pod_status[first_key].message}")
        on_node = sorted(p.key for n, p in batch if n == first_node and
                         int(res[[q.key for _, q in batch].index(p.key)]) == abi.KG_BATCH_ROLLED_BACK)
        if on_node:
            msg += f", assumed pods on node {first_node}: " + ", ".join(on_node)
        for key in pod_status:
            if pod_status[key].is_success():
                pod_status[key] = Status(UNSCHEDULABLE, JOB_SCHEDULE_FAILED)
        return JobOutcome(Status(UNSCHEDULABLE, msg), pod_status, {})
