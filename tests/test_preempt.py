"""kg_eval_preempt on the device: SelectVictimsOnNode (elasticquota/preempt.go:111-217, reservation/preemption.go:
123-219) of 8 preemptors on every node, against the loop rebuilt from the CPU oracle (preempt_ref).

Bar: exact (np.array_equal) on every field of kg_preempt_node and on the victim masks of the CANDIDATE nodes (the
others' masks are all zero on both sides), no node left out. The inputs of `small` and `mixed` are shown, from the
reference alone, to tell the loop from three wrong readings (no reprieve, reprieve from the least important pod,
budgets ignored) and to hold every result kind. Measured on the CPU with the seeds of preempt_ref.SEEDS (distinct nodes,
flags 0): small: 186 / 34 / 16 nodes differ from the readings, 187 CANDIDATE, 299 NO_VICTIMS, 146 NO_FIT, 64
UNSUPPORTED, 31 with two or more victims, 10 with violating victims; mixed: 122 / 20 / 9, 123, 240, 115, 68, 11, 7."""
import ctypes as C
import functools

import numpy as np
import pytest

import node_sets_ref as sets_ref
import oracle_lib
import preempt_ref as ref
from koordinator_amd import abi, engine, synth

pytestmark = pytest.mark.gpu

CLUSTERS = ("small", "mixed", "n129", "n33", "topology")
BOTH = abi.KG_PREEMPT_SKIP_NON_PREEMPTIBLE | abi.KG_PREEMPT_SAME_GROUP
FLAGS = (0, abi.KG_PREEMPT_SKIP_NON_PREEMPTIBLE, BOTH)
FIELDS = [f for f in abi.PREEMPT_NODE_DTYPE.names if f != "pad_"]


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def case(name):
    """The inputs of one cluster (preempt_ref.case_inputs); read-only."""
    return ref.case_inputs(name, synth)


@functools.lru_cache(maxsize=None)
def want(name, flags=0):
    c = case(name)
    out, vic = ref.preempt(c["kc"], c["nodes"], c["pods"], c["res"], c["rows"], c["priority"], c["group"], flags=flags)
    out.setflags(write=False)
    vic.setflags(write=False)
    return out, vic


def make(ctx, name, index_base=0):
    c = case(name)
    snap = engine.Snapshot(ctx, c["kc"], c["nodes"], index_base)
    snap.upload_residents(c["res"])
    return snap, engine.PodBatch(ctx, c["pods"])


def run(snap, pb, c, flags=0, **kw):
    return engine.eval_preempt(snap, pb, c["rows"], c["priority"], c["group"], ref.ALLOWED, flags, victims=True, **kw)


def check(got, exp, what):
    out, vic = got
    assert out.dtype == abi.PREEMPT_NODE_DTYPE and out.shape == exp[0].shape and vic.shape == exp[1].shape, what
    for f in FIELDS:
        assert np.array_equal(out[f], exp[0][f]), (what, f, np.argwhere(out[f] != exp[0][f])[:6])
    assert not out["pad_"].any()
    cand = exp[0]["result"] == abi.KG_PREEMPT_CANDIDATE
    assert np.array_equal(vic[cand], exp[1][cand]), (what, "victim masks")
    assert not vic[~cand].any(), (what, "masks of nodes that are no candidates")


# ---- 1. parity ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CLUSTERS)
def test_parity(ctx, name):
    c = case(name)
    if name in ("small", "mixed"):  # from the reference alone: the inputs discriminate
        d = ref.discrimination(c)
        print(f"{name}: {d}")
        assert min(d.values()) >= 5, d
    snap, pb = make(ctx, name)
    for flags in FLAGS:
        exp = want(name, flags)
        check(run(snap, pb, c, flags), exp, (name, flags))
        got = engine.eval_preempt(snap, pb, c["rows"], c["priority"], c["group"], ref.ALLOWED, flags)
        for f in FIELDS:
            assert np.array_equal(got[f], exp[0][f]), (name, flags, f, "without the victim masks")
    # positions map back to upload rows
    count, row = snap.read_residents()
    lists = ref.node_lists(c["res"], snap.n)
    assert np.array_equal(count, [len(l) for l in lists]) and np.array_equal(row, np.concatenate(lists))


def test_overflowed_list_and_group_none(ctx):
    c = case("small")
    i = ref.OVERFLOW_NODE["small"]
    exp = want("small")
    assert (exp[0]["result"][:, i] == abi.KG_PREEMPT_UNSUPPORTED).all() and (exp[0]["status"][:, i] == abi.KG_ST_UNSUPPORTED).all()
    snap, pb = make(ctx, "small")
    # group None means -1 for every preemptor
    e2 = ref.preempt(c["kc"], c["nodes"], c["pods"], c["res"], c["rows"], c["priority"], None, flags=BOTH)
    got = engine.eval_preempt(snap, pb, c["rows"], c["priority"], None, ref.ALLOWED, BOTH, victims=True)
    check(got, e2, "group None")
    assert not np.array_equal(e2[0]["result"], want("small", BOTH)[0]["result"])


# ---- 2. candidate node sets --------------------------------------------------------------------------------------
def test_with_node_sets(ctx):
    c = case("small")
    ver = oracle_lib.eval_verify(c["kc"], c["nodes"], c["pods"])
    mask, pod_set, bits, kind = sets_ref.kind_masks(ver.status, ver.total)
    snap, pb = make(ctx, "small")
    pb.set_node_sets(pod_set, bits, snap.n)
    exp = ref.preempt(c["kc"], c["nodes"], c["pods"], c["res"], c["rows"], c["priority"], c["group"], mask=mask)
    excl = exp[0]["result"] == abi.KG_PREEMPT_EXCLUDED
    assert excl.sum() >= 50 and (~excl).sum() >= 50, (excl.sum(), "pairs excluded")
    assert (exp[0]["status"][excl] == abi.KG_ST_NODE_EXCLUDED).all() and not exp[0]["n_potential"][excl].any()
    check(run(snap, pb, c), exp, "with sets")
    pb.clear_node_sets()
    check(run(snap, pb, c), want("small"), "sets cleared")


# ---- 3. nothing changes ------------------------------------------------------------------------------------------
def test_nothing_changes(ctx):
    c = case("small")
    snap, pb = make(ctx, "small")
    keys = engine.eval_select(snap, pb, 3)
    status = engine.result_status(pb)
    gen = snap.generation()
    state = snap.read_state()
    check(run(snap, pb, c), want("small"), "small")
    assert np.array_equal(engine.result_keys(pb, 3), keys)
    assert np.array_equal(engine.result_status(pb), status)
    assert snap.generation() == gen
    after = snap.read_state()
    assert state.keys() == after.keys()
    for k in state:
        assert np.array_equal(state[k], after[k]), k
    assert np.array_equal(engine.eval_select(snap, pb, 3), oracle_lib.select(c["kc"], c["nodes"], c["pods"], 3))
    # the resident calls bump the generation; a node upload drops the table
    snap.upload_residents(c["res"])
    assert snap.generation() == gen + 1
    snap.upload(c["nodes"])
    with pytest.raises(engine.EngineError) as e:
        run(snap, pb, c)
    assert e.value.status == abi.KG_INVALID_ARG and "resident" in str(e.value)


# ---- 4. layout, updates and shards -------------------------------------------------------------------------------
def test_after_rows_moved_between_storage_classes(ctx):
    c = case("small")
    nodes = c["nodes"]
    snap, pb = make(ctx, "small")
    check(run(snap, pb, c), want("small"), "before")
    single = np.flatnonzero(nodes["numa_policy"] == abi.KG_NUMA_SINGLE_NODE)
    other = np.flatnonzero(nodes["numa_policy"] != abi.KG_NUMA_SINGLE_NODE)
    rows = np.array(sorted({int(single[0]), int(other[0]), int(other[-1])}), np.uint32)
    upd = abi.take(nodes, rows.astype(np.int64))
    upd["numa_policy"] = np.where(upd["numa_policy"] == abi.KG_NUMA_SINGLE_NODE, abi.KG_NUMA_NONE,
                                  abi.KG_NUMA_SINGLE_NODE).astype(np.uint32)
    snap.update_rows(rows, upd)  # three nodes move to the other storage class: every record between them shifts
    merged = {k: (v if k in abi.TABLE_KEYS else v.copy()) for k, v in nodes.items()}
    for k in upd:
        if k not in abi.TABLE_KEYS:
            merged[k][rows] = upd[k]
    exp = ref.preempt(c["kc"], merged, c["pods"], c["res"], c["rows"], c["priority"], c["group"])
    check(run(snap, pb, c), exp, "after the update: the table stays with the positions")


def test_update_residents_equals_upload_of_the_merged_table(ctx):
    c = case("small")
    res = c["res"]
    snap, pb = make(ctx, "small")
    picked = np.array([3, 150, 299], np.uint32)
    # node 3 gets its own rows back reversed with new priorities, node 150 ends up empty, node 299 takes node 5's pods
    a = {k: v[res["node"] == 3][::-1].copy() for k, v in res.items()}
    a["priority"] = np.roll(a["priority"], 1)
    b = {k: v[res["node"] == 5].copy() for k, v in res.items()}
    b["node"][:] = 299
    upd = {k: np.concatenate([a[k], b[k]]) for k in res}
    gen = snap.generation()
    snap.update_residents(picked, upd)
    assert snap.generation() == gen + 1
    merged = ref.merge(res, picked, upd)
    exp = ref.preempt(c["kc"], c["nodes"], c["pods"], merged, c["rows"], c["priority"], c["group"])
    assert any(not np.array_equal(exp[0][f], want("small")[0][f]) for f in FIELDS)
    got = run(snap, pb, c)
    check(got, exp, "after update_residents")
    count, row = snap.read_residents()
    assert count[150] == 0 and count[3] == len(a["node"]) and count[299] == len(b["node"])
    # Updates append to a spare tail behind the table (16k entries at least) and lay the table out again when it is used
    # up: 70 updates of 250 entries cross that point; then node 7 gets its own list back (the same rows, a new order)
    junk = abi.empty_residents(250)
    junk["node"][:] = 7
    for k in range(70):
        junk["priority"][:] = k
        snap.update_residents([7], junk)
    assert snap.read_residents()[0][7] == 250 and snap.generation() == gen + 71
    back = {k: v[merged["node"] == 7].copy() for k, v in merged.items()}
    snap.update_residents([7], back)
    merged = ref.merge(merged, [7], back)
    got = run(snap, pb, c)
    check(got, exp, "after the tail was used up and the table laid out again")
    count, row = snap.read_residents()
    assert np.array_equal(count, [len(l) for l in ref.node_lists(merged, snap.n)])
    full = engine.Snapshot(ctx, c["kc"], c["nodes"])
    full.upload_residents(merged)
    got2 = run(full, pb, c)
    for f in abi.PREEMPT_NODE_DTYPE.names:
        assert np.array_equal(got[0][f], got2[0][f]), f
    assert np.array_equal(got[1], got2[1])


def test_shards_concatenate_and_index_base_is_not_added(ctx):
    c = case("small")
    n = abi.table_len(c["nodes"])
    pb = engine.PodBatch(ctx, c["pods"])
    outs, vics = [], []
    for idx in (np.arange(0, 150), np.arange(150, n)):
        snap = engine.Snapshot(ctx, c["kc"], abi.take(c["nodes"], idx), int(idx[0]))
        sel = np.isin(c["res"]["node"], idx)
        part = {k: v[sel].copy() for k, v in c["res"].items()}
        part["node"] = (part["node"] - idx[0]).astype(np.uint32)
        snap.upload_residents(part)
        o, v = run(snap, pb, c)
        outs.append(o)
        vics.append(v)
    check((np.concatenate(outs, axis=1), np.concatenate(vics, axis=1)), want("small"), "halves")
    snap, pb = make(ctx, "small", index_base=1000)
    check(run(snap, pb, c), want("small"), "index_base 1000")


# ---- 5. arguments and refusals -----------------------------------------------------------------------------------
def test_arguments(ctx):
    c = case("n129")
    snap, pb = make(ctx, "n129")
    L = ctx.L
    PN, PU, PI = C.POINTER(abi.KgPreemptNode), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
    R, n, W = len(c["rows"]), snap.n, abi.KG_PREEMPT_MASK_WORDS
    rows, prio, allowed = c["rows"], c["priority"], ref.ALLOWED
    rp, pp, ap = rows.ctypes.data_as(PU), prio.ctypes.data_as(PI), allowed.ctypes.data_as(PI)
    out = np.zeros(R * n + 1, abi.PREEMPT_NODE_DTYPE)
    op = out.ctypes.data_as(PN)
    res = c["res"]
    bad_node = {k: v[:4].copy() for k, v in res.items()}
    bad_node["node"][2] = n
    bad_pdb = {k: v[:4].copy() for k, v in res.items()}
    bad_pdb["pdb1"][1] = -2
    null_col = abi.resident_columns({k: v[:4].copy() for k, v in res.items()})
    null_col.start_time = None
    stray = {k: v[res["node"] == 7].copy() for k, v in res.items()}
    bad = [
        lambda: ctx.check(L.kg_eval_preempt(snap.h, pb.h, rp, R, pp, None, ap, len(allowed), 0, None, None), "null out"),
        lambda: ctx.check(L.kg_eval_preempt(snap.h, pb.h, rp, R, None, None, ap, len(allowed), 0, op, None), "null priority"),
        lambda: ctx.check(L.kg_eval_preempt(snap.h, pb.h, rp, R, pp, None, None, len(allowed), 0, op, None), "null allowed"),
        lambda: ctx.check(L.kg_eval_preempt(snap.h, pb.h, rp, R, pp, None, ap, len(allowed) - 1, 0, op, None), "n_pdbs too small"),
        lambda: ctx.check(L.kg_eval_preempt(snap.h, pb.h, rp, R, pp, None, ap, len(allowed), 4, op, None), "unknown flag"),
        lambda: ctx.check(L.kg_eval_preempt(snap.h, pb.h, None, R, pp, None, ap, len(allowed), 0, op, None), "n_rows"),
        lambda: engine.eval_preempt(snap, pb, [pb.n], [5], None, allowed),
        lambda: snap.upload_residents(bad_node),
        lambda: snap.upload_residents(bad_pdb),
        lambda: ctx.check(L.kg_snapshot_upload_residents(snap.h, C.byref(null_col), 4), "null column"),
        lambda: snap.update_residents([n], abi.empty_residents(0)),
        lambda: snap.update_residents([3, 3], abi.empty_residents(0)),
        lambda: snap.update_residents([3], stray),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(engine.EngineError) as ei:
            call()
        assert ei.value.status == abi.KG_INVALID_ARG, k
    exp = want("n129")
    check(run(snap, pb, c), exp, "the refused calls changed nothing")
    # guard words behind the outputs of a full call stay intact; n_rows == 0 writes nothing
    raw = np.full(R * n * 8 + 8, 0xDEADBEEF, np.uint32)  # 32 bytes per pair and one pair of guard
    vic = np.full(R * n * W + 2, 0xDEADBEEF, np.uint32)
    ctx.check(L.kg_eval_preempt(snap.h, pb.h, rp, 0, pp, None, ap, len(allowed), 0, raw.ctypes.data_as(PN),
                                vic.ctypes.data_as(PU)), "0 rows")
    assert (raw == 0xDEADBEEF).all() and (vic == 0xDEADBEEF).all()
    got0 = engine.eval_preempt(snap, pb, [], [], None, allowed, victims=True)
    assert got0[0].shape == (0, n) and got0[1].shape == (0, n, W)
    gp = c["group"].ctypes.data_as(PI)
    ctx.check(L.kg_eval_preempt(snap.h, pb.h, rp, R, pp, gp, ap, len(allowed), 0, raw.ctypes.data_as(PN),
                                vic.ctypes.data_as(PU)), "guarded")
    assert (raw[R * n * 8:] == 0xDEADBEEF).all() and (vic[R * n * W:] == 0xDEADBEEF).all()
    check((raw[:R * n * 8].view(abi.PREEMPT_NODE_DTYPE).reshape(R, n), vic[:R * n * W].reshape(R, n, W)), exp, "guarded")


def test_snapshot_of_no_nodes(ctx):
    c = case("n33")
    snap0 = engine.Snapshot(ctx, c["kc"], abi.take(c["nodes"], np.zeros(0, np.int64)))
    snap0.upload_residents(abi.empty_residents(0))
    pb = engine.PodBatch(ctx, c["pods"])
    guard = np.full(16, 0xDEADBEEF, np.uint32)
    L = ctx.L
    PN, PU, PI = C.POINTER(abi.KgPreemptNode), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
    ctx.check(L.kg_eval_preempt(snap0.h, pb.h, c["rows"].ctypes.data_as(PU), len(c["rows"]), c["priority"].ctypes.data_as(PI),
                                None, ref.ALLOWED.ctypes.data_as(PI), len(ref.ALLOWED), 0, guard.ctypes.data_as(PN),
                                guard[8:].ctypes.data_as(PU)), "0 nodes")
    assert (guard == 0xDEADBEEF).all()
    got = run(snap0, pb, c)
    assert got[0].shape == (len(c["rows"]), 0) and got[1].shape == (len(c["rows"]), 0, abi.KG_PREEMPT_MASK_WORDS)
    count, row = snap0.read_residents()
    assert count.shape == (0,) and row.shape == (0,)


def test_refusals(ctx):
    c = case("n33")
    snap = engine.Snapshot(ctx, c["kc"], c["nodes"])
    pb = engine.PodBatch(ctx, c["pods"])
    with pytest.raises(engine.EngineError) as e:  # no residents uploaded
        run(snap, pb, c)
    assert e.value.status == abi.KG_INVALID_ARG and "resident" in str(e.value)
    with pytest.raises(engine.EngineError) as e:
        snap.update_residents([0], abi.empty_residents(0))
    assert e.value.status == abi.KG_INVALID_ARG
    cfg, nodes, pods, quotas, rsv = synth.cluster5(64, 16, seed_config=12)
    kc = cfg.kg_config()
    snap5 = engine.Snapshot(ctx, kc, nodes)
    snap5.upload_quotas(quotas)
    if kc.plugins & abi.KG_PLUGIN_RSV:
        snap5.upload_reservations(rsv)
    snap5.upload_residents(abi.empty_residents(0))
    pb5 = engine.PodBatch(ctx, pods)
    with pytest.raises(engine.Unsupported) as e:
        engine.eval_preempt(snap5, pb5, [0, 1], [100, 100], None, ref.ALLOWED)
    assert e.value.status == abi.KG_UNSUPPORTED and "config-5" in str(e.value)
    snap.upload_residents(c["res"])
    check(run(snap, pb, c), want("n33"), "a plain call afterwards")
