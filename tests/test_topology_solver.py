"""The host side of the network-topology planner (koordinator_amd.batch.place_pods and its parts; no device) against the
tables of the reference's network_topology_solver_test.go, transcribed as data in tests/golden/topology_solver_kat.json.
Every expectation there carries "ref" (asserted by the cited reference test) or "derived": true (worked out by hand from
network_topology_solver.go); test_kat_labels counts both kinds. Beside the tables: the failure message, a job that fits
only at a higher layer, and the independence from the order children were inserted in (the reference iterates a Go
map and sorts)."""
import json
import os
import random

import pytest

from koordinator_amd import abi, batch
from koordinator_amd.batch import JobPod, JobTopologyRequirements, TopologyNode

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "topology_solver_kat.json")) as f:
    KAT = json.load(f)
NODE = batch.NODE_TOPOLOGY_LAYER


def build(tree):
    """{name: TopologyNode} of one of the KAT's trees (parents listed before their children)."""
    nodes = {}
    for d in KAT["trees"][tree]:
        n = TopologyNode(d["layer"], d["name"], offer_slot=d.get("offer_slot", 0), score=d.get("score", 0),
                         existing_pod_num=d.get("existing_pod_num", 0))
        if d["parent"] is not None:
            nodes[d["parent"]].add_child(n)
        nodes[n.name] = n
    return nodes


def ident(case):
    return case["name"]


def test_kat_labels():
    n_ref = n_derived = 0
    for table in ("less", "distribute", "constrain"):
        for case in KAT[table]:
            assert ("ref" in case) != bool(case.get("derived")), case["name"]
            n_ref += "ref" in case
            n_derived += bool(case.get("derived"))
    print(f"topology solver KAT: {n_ref} ref, {n_derived} derived expectations")
    assert n_ref == 19 and n_derived == 5


@pytest.mark.parametrize("case", KAT["less"], ids=ident)
def test_topology_node_less(case):
    nodes = build(case["tree"])
    assert batch.topology_node_less(nodes[case["a"]], nodes[case["b"]], case["lower"]) is case["want"], \
        case.get("ref", "derived")


@pytest.mark.parametrize("case", KAT["distribute"], ids=ident)
def test_distribute_offer_slot(case):
    nodes = build(case["tree"])
    distribution = {}
    order, total = batch.distribute_offer_slot(case["desired"], nodes[case["at"]], distribution, case["multiples"] or None)
    assert total == case["want_total"], case.get("ref", "derived")
    if "want_distribution" in case:
        assert distribution == case["want_distribution"], case.get("ref", "derived")
    if "want_order" in case:
        assert order == case["want_order"]
    assert sum(distribution.values()) == total


@pytest.mark.parametrize("case", KAT["constrain"], ids=ident)
def test_constrain_offer_slot_by_pod_count_multiple(case):
    nodes = build(case["tree"])
    batch.constrain_offer_slot_by_pod_count_multiple(nodes["s1"], case["multiples"] or None)
    assert {k: nodes[k].offer_slot for k in case["want_offer_slots"]} == case["want_offer_slots"], case["ref"]


# ---- place_pods -------------------------------------------------------------------------------------------------------
def cluster(order=None):
    """cluster -> spines s1 {b1 {n1, n2}, b2 {n3, n4}}, s2 {b3 {n5, n6}}; `order`: a shuffle of the insertions."""
    edges = [("cluster", "s1", "SpineLayer"), ("cluster", "s2", "SpineLayer"), ("s1", "b1", "BlockLayer"),
             ("s1", "b2", "BlockLayer"), ("s2", "b3", "BlockLayer"), ("b1", "n1", NODE), ("b1", "n2", NODE),
             ("b2", "n3", NODE), ("b2", "n4", NODE), ("b3", "n5", NODE), ("b3", "n6", NODE)]
    made = {"cluster": TopologyNode("ClusterLayer", "cluster")}
    for _, name, layer in edges:
        made[name] = TopologyNode(layer, name)
    links = list(edges)
    if order is not None:
        order.shuffle(links)
    for parent, name, _ in links:
        made[parent].add_child(made[name])
    return made["cluster"]


SLOTS = {"n1": 2, "n2": 1, "n3": 3, "n4": 0, "n5": 2, "n6": 2}


def gang(n):
    return [JobPod("ns", f"p{j:02d}") for j in range(n)]


def test_place_in_the_lowest_holding_layer():
    # 3 pods: blocks b1 (3), b2 (3) and b3 (4) hold them, no single node but n3 does: the node layer wins, n3 alone
    plan, msg = batch.place_pods(cluster(), SLOTS, JobTopologyRequirements("SpineLayer", 3), gang(3))
    assert msg == "" and plan == {"ns/p00": "n3", "ns/p01": "n3", "ns/p02": "n3"}
    # 4 pods: only block b3 holds them (lower slot first is moot), its larger-or-equal node by name first
    plan, msg = batch.place_pods(cluster(), SLOTS, JobTopologyRequirements("SpineLayer", 4), gang(4))
    assert msg == "" and plan == {"ns/p00": "n5", "ns/p01": "n5", "ns/p02": "n6", "ns/p03": "n6"}


def test_job_that_fits_only_at_a_higher_layer():
    # 5 pods: no block holds them, spine s1 (6) does; its blocks tie at 3, b1 by name, n1 (2) before n2 (1); then b2's n3
    plan, msg = batch.place_pods(cluster(), SLOTS, JobTopologyRequirements("SpineLayer", 5), gang(5))
    assert msg == ""
    assert plan == {"ns/p00": "n1", "ns/p01": "n1", "ns/p02": "n2", "ns/p03": "n3", "ns/p04": "n3"}
    # 7 pods: no spine holds them; without a must-gather layer the cluster (10) does, the larger spine first
    assert batch.place_pods(cluster(), SLOTS, JobTopologyRequirements("SpineLayer", 7), gang(7))[0] is None
    plan, msg = batch.place_pods(cluster(), SLOTS, JobTopologyRequirements("", 7), gang(7))
    assert msg == "" and sorted(plan.values()) == ["n1", "n1", "n2", "n3", "n3", "n3", "n5"]


def test_existing_pods_order_the_candidates():
    req = JobTopologyRequirements("SpineLayer", 3)
    slots = dict(SLOTS, n3=2)  # no node holds 3; of the blocks b1 (3), b2 (2), b3 (4) b1 has the lower slot: first
    plan, _ = batch.place_pods(cluster(), slots, req, gang(3))
    assert set(plan.values()) == {"n1", "n2"}
    plan, _ = batch.place_pods(cluster(), slots, req, gang(3), existing_pod_num={"n6": 2})
    assert plan == {"ns/p00": "n6", "ns/p01": "n6", "ns/p02": "n5"}  # the node with the job's pods first


def test_no_candidate_message():
    req = JobTopologyRequirements("BlockLayer", 5, {"BlockLayer": 2, NODE: 2})
    status = {"n1": abi.KG_ST_NRF_CPU | abi.KG_ST_LA_CPU, "n2": abi.KG_ST_NRF_CPU, "n3": abi.KG_ST_LA_EXPIRED,
              "n4": abi.KG_ST_NRF_MEM, "n5": 0}
    plan, msg = batch.place_pods(cluster(), SLOTS, req, gang(5), node_status=status)
    assert plan is None
    # node multiple 2: n1 2, n2 0, n3 2, n4 0, n5 2, n6 2 -> blocks 2, 2, 4; n1's word counts under its first plugin only
    assert msg == ("no candidate topology nodes can accommodate job, desiredOfferSlot: 5, "
                   "topology topologyNode BlockLayer/b1: 2;topology topologyNode BlockLayer/b2: 2;"
                   "topology topologyNode BlockLayer/b3: 4, "
                   "0/6 nodes are available: 1 Insufficient memory, 1 node(s) nodeMetric expired, 2 Insufficient cpu."
                   "; podCountMultiple constraints: BlockLayer=2, NodeTopologyLayer=2")
    # a must-gather layer the tree does not have: no topology node listed, no multiples tail
    plan, msg = batch.place_pods(cluster(), SLOTS, JobTopologyRequirements("RackLayer", 1), gang(1), num_all_nodes=9)
    assert plan is None
    assert msg == "no candidate topology nodes can accommodate job, desiredOfferSlot: 1, , 0/9 nodes are available:"


def test_child_insertion_order_does_not_matter():
    req = JobTopologyRequirements("", 7, {NODE: 1})
    want = batch.place_pods(cluster(), SLOTS, req, gang(7), node_to_score={"n5": 3})
    assert want[0] is not None
    for seed in range(8):
        assert batch.place_pods(cluster(random.Random(seed)), SLOTS, req, gang(7), node_to_score={"n5": 3}) == want


def test_place_pods_leaves_the_tree_alone():
    root = cluster()
    batch.place_pods(root, SLOTS, JobTopologyRequirements("", 4), gang(4), existing_pod_num={"n1": 1},
                     node_to_score={"n1": 5})
    for node in batch.enumerate_node_topology_nodes(root).values():
        while node is not None:
            assert (node.offer_slot, node.score, node.existing_pod_num) == (0, 0, 0)
            node = node.parent


def test_pods_are_dealt_by_name():
    pods = [JobPod("ns", "b"), JobPod("ns", "c"), JobPod("ns", "a")]
    plan, _ = batch.place_pods(cluster(), {"n1": 1, "n2": 2}, JobTopologyRequirements("", 3), pods)
    assert plan == {"ns/a": "n2", "ns/b": "n2", "ns/c": "n1"}
