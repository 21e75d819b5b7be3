"""Host side of the node offer slots (kg_eval_offer_slots; no device): the agreement of include/koordgpu.h and abi.py on
the new symbol within ABI 14, and batch.place_pods against a brute-force enumeration on random small trees."""
import ctypes as C
import os
import random
import re

from koordinator_amd import abi, batch
from koordinator_amd.batch import JobPod, JobTopologyRequirements, TopologyNode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "koordgpu.h")
NODE = batch.NODE_TOPOLOGY_LAYER

CTYPE = {"kg_snap*": C.c_void_p, "kg_pods*": C.c_void_p, "const uint32_t*": C.POINTER(C.c_uint32),
         "uint32_t*": C.POINTER(C.c_uint32), "uint32_t": C.c_uint32}


def header():
    with open(HEADER) as f:
        return f.read()


def test_header_declares_the_call_within_abi_14():
    src = header()
    assert re.search(r"^kg_status kg_eval_offer_slots\(kg_snap\* snap, kg_pods\* pods, const uint32_t\* rows, "
                     r"uint32_t n_rows,\s*uint32_t\* out_slots /\* n_nodes \*/, uint32_t\* out_status /\* n_nodes, may be "
                     r"NULL \*/\);", src, re.M)
    assert re.search(r"^#define KG_ABI_VERSION 14\b", src, re.M) and abi.KG_ABI_VERSION == 14
    # the refusal names its cause
    doc = src[:src.index("kg_status kg_eval_offer_slots(")]
    doc = doc[doc.rindex("/*"):]
    assert "KG_UNSUPPORTED" in doc and "Reservation's AddPod" in doc and "KG_PLUGIN_EXT" in doc


def test_abi_signature_matches_the_prototype():
    m = re.search(r"^kg_status kg_eval_offer_slots\((.*?)\);", header(), re.M | re.S)
    assert m
    params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    types = [re.sub(r"\s*\w+$", "", p) for p in params]  # drop the parameter name
    assert types == ["kg_snap*", "kg_pods*", "const uint32_t*", "uint32_t", "uint32_t*", "uint32_t*"]
    assert [CTYPE[t] for t in types] == abi.KG_EVAL_OFFER_SLOTS_ARGTYPES


# ---- place_pods against a brute force -----------------------------------------------------------------------------------
LAYERS = ("ClusterLayer", "SpineLayer", "BlockLayer")


def random_tree(rng):
    """(root, leaves [(path of ancestor names from the root, leaf name)]) with 1..3 layers above at most 12 leaves."""
    depth = rng.randint(1, 3)
    root = TopologyNode(LAYERS[0], "cluster")
    level = [(root, ("cluster",))]
    for d in range(1, depth):
        nxt = []
        for node, path in level:
            for _ in range(rng.randint(1, 3)):
                name = f"{LAYERS[d][0].lower()}{len(nxt)}"
                nxt.append((node.add_child(TopologyNode(LAYERS[d], name)), path + (name,)))
        level = nxt
    leaves = []
    budget = 12
    for at, (node, path) in enumerate(level):
        for _ in range(rng.randint(1, max(1, min(3, budget - (len(level) - at - 1))))):
            name = f"n{len(leaves):02d}"
            node.add_child(TopologyNode(NODE, name))
            leaves.append((path, name))
            budget -= 1
    assert len(leaves) <= 12
    return root, leaves, depth


def brute_force(leaves, depth, slots, existing, scores, must_depth, desired):
    """The topology node (path) the solver must choose, or None: of the topology nodes at or below the must-gather
    depth, the deepest layer with a node holding the job; there the first in topologyNodeLessFunc's order."""
    def total(table, prefix):
        return sum(table.get(name, 0) for path, name in leaves if (path + (name,))[:len(prefix)] == prefix)

    best = None
    for d in range(must_depth, depth + 2):  # depth + 1 = the node layer
        prefixes = sorted({(path + (name,))[:d] for path, name in leaves})
        holding = [p for p in prefixes if total(slots, p) >= desired]
        if not holding:
            break  # a child holds no more than its parent
        def key(p):
            chain = [p[:k] for k in range(len(p), 0, -1)]
            return (tuple(-total(existing, c) for c in chain), tuple(total(slots, c) for c in chain),
                    -total(scores, p), p[-1])
        best = min(holding, key=key)
    return best


def test_place_pods_agrees_with_brute_force():
    rng = random.Random(20)
    placed = refused = 0
    for _ in range(300):
        root, leaves, depth = random_tree(rng)
        names = [name for _, name in leaves]
        slots = {n: rng.choice([0, 0, 1, 2, 3, 5]) for n in names}
        existing = {n: rng.choice([0, 0, 0, 1, 2]) for n in names}
        scores = {n: rng.choice([0, 10, 20]) for n in names}
        must_depth = rng.randint(1, depth)  # 1 = the root: no must-gather layer
        desired = rng.randint(1, 9)
        req = JobTopologyRequirements("" if must_depth == 1 else LAYERS[must_depth - 1], desired)
        pods = [JobPod("ns", f"p{j}") for j in range(desired)]
        plan, msg = batch.place_pods(root, slots, req, pods, existing, scores)
        want = brute_force(leaves, depth, slots, existing, scores, must_depth, desired)
        if want is None:
            assert plan is None and msg.startswith("no candidate topology nodes can accommodate job, desiredOfferSlot: "
                                                   f"{desired}, ")
            refused += 1
            continue
        placed += 1
        assert plan is not None and sorted(plan) == sorted(p.key for p in pods)
        full = {name: path + (name,) for path, name in leaves}
        for node in set(plan.values()):
            assert full[node][:len(want)] == want, (node, want)
            assert list(plan.values()).count(node) <= slots[node]
    assert placed >= 60 and refused >= 60, (placed, refused)
