// kg_rowfilter.h — the Filter status word of a (batch row, node record) pair for the row-list evaluators: kg_eval_diagnose
// (kg_diag.hip), kg_eval_feasible (kg_feasible.hip), kg_eval_offer_slots (kg_slots.hip) and kg_eval_preempt
// (kg_preempt.hip). Internal to libkoordgpu.so.
//
// The word is kg_eval_verify's bit for bit: the plain plugin set evaluates a pair with eval_pair (filters only: no
// score, no zone), the config-5 set with eval_pair_ext behind the ElasticQuota gate, and a record outside the pod's
// candidate node set takes KG_ST_NODE_EXCLUDED beside its word. The host part describes such a launch (RowFilter), says
// whether it may run (rowfilter_valid) and picks the instantiation (rowfilter_dispatch); the device part (HIP
// translation units only) is the lane's row context (RowCtx, RowSet) and row_status. What a kernel does with the word,
// and when it loads the candidate word of a 64-record block, stays the kernel's.
#pragma once
#include <hip/hip_runtime_api.h>

#include <type_traits>

#include "kg_kernels.h"
#include "kg_sets.h"

namespace kg {

// One row-list Filter launch over every record of a snapshot. The record-order table holds sets_words(n_nodes) words
// per set (kg_sets.h).
struct RowFilter {
    const NodeRec* nodes;
    const ZoneRec* zones;
    uint32_t n_nodes;
    KCfg cfg;
    bool exact;
    bool ext;             // the snapshot carries the config-5 tables: e, and qst = the ElasticQuota gate's status per pod
    ExtDev e;             // (launch_ext_gate, on the same stream before the launch)
    const uint32_t* qst;
    PodsDev pods;
    const uint32_t* rows;  // device copy of the caller's list; nullptr: row t is pod t
    uint32_t n_rows;
    const int32_t* pod_set;  // nullable (plain snapshots only): the batch carries candidate node sets,
    const uint64_t* tab;     // tab their record-order table
};

inline bool rowfilter_valid(const RowFilter& f) {
    return f.nodes && f.zones && !(f.pod_set && (f.ext || !f.tab)) && !(f.ext && !f.qst);
}

// launch(exact, ext, sets) with std::bool_constants for a valid f. Candidate node sets are not served on config-5
// snapshots: no EXT-and-SETS form exists. WITH_EXT = false (a caller that refuses f.ext itself) instantiates no EXT
// form either.
template <bool WITH_EXT = true, class Launch>
inline void rowfilter_dispatch(const RowFilter& f, Launch&& launch) {
    const auto by_exact = [&](auto ext, auto sets) {
        if (f.exact) launch(std::true_type{}, ext, sets);
        else launch(std::false_type{}, ext, sets);
    };
    if (f.pod_set) return by_exact(std::false_type{}, std::true_type{});
    if constexpr (WITH_EXT)
        if (f.ext) return by_exact(std::true_type{}, std::false_type{});
    by_exact(std::false_type{}, std::false_type{});
}

}  // namespace kg

#ifdef __HIPCC__
#include "kg_cpuset_reserve.h"
#include "kg_ext.h"
#include "kg_ext_wave.h"

namespace kg {

// What a lane keeps of its row (pod j of the batch) while it walks records.
struct RowCtx {
    PodV p;
    PodX px;     // EXT only
    uint32_t q;  // EXT only: the ElasticQuota gate's status of the pod
    const ExtDev* e;
};

// live = false: an idle lane that walks the records along with its wave. It takes q = 1 (decided, no pair evaluated).
// Without EXT e may be nullptr and qst is not read.
template <bool EXT>
__device__ __forceinline__ RowCtx row_ctx(const PodsDev& pods, uint32_t j, bool live, const ExtDev* e,
                                          const uint32_t* __restrict__ qst) {
    RowCtx c{};
    c.p = load_pod(pods, j);
    c.e = e;
    if constexpr (EXT) {
        c.px = load_podx(pods, j);
        c.q = live ? qst[j] : 1u;
    }
    return c;
}

// The row's candidate node set: its id (-1 = none) and its row of the record-order table. Kept beside RowCtx, not in
// it: a kernel that needs the set once (k_feasible_by_records) fetches it after the evaluation, where it is live
// across nothing. Without SETS pod_set and tab are not read.
struct RowSet {
    int32_t set;
    const uint64_t* srow;
};
template <bool SETS>
__device__ __forceinline__ RowSet row_set(const int32_t* __restrict__ pod_set, const uint64_t* __restrict__ tab,
                                          uint32_t words, uint32_t j) {
    if constexpr (SETS) {
        const int32_t set = pod_set[j];
        return {set, set >= 0 ? tab + (size_t)set * words : tab};
    } else {
        return {-1, nullptr};
    }
}

// The row's candidate word for the 64-record block of rec (a pod without a set: all ones).
__device__ __forceinline__ uint64_t row_cand(const RowSet& rs, uint32_t rec) {
    return rs.set >= 0 ? rs.srow[rec >> 6] : ~0ull;
}

// st, with KG_ST_NODE_EXCLUDED where rec lies outside the row's candidate set (cand: row_cand of rec's block).
__device__ __forceinline__ uint32_t row_exclude(uint32_t st, uint64_t cand, uint32_t rec) {
    return st | (((cand >> (rec & 63u)) & 1ull) ? 0u : (uint32_t)KG_ST_NODE_EXCLUDED);
}

// The same for a kernel that evaluates one pair of the row and so has no block to keep the word for.
__device__ __forceinline__ uint32_t row_exclude(uint32_t st, const RowSet& rs, uint32_t rec) {
    return rs.set >= 0 ? row_exclude(st, rs.srow[rec >> 6], rec) : st;
}

// The pair's status word. n: the record's slots (nodes[rec].v, or a staged copy of its int section and flag word);
// cand: row_cand of rec's block (read with SETS only); OV: the slots of ov override the record's (kg_eval.h), plain
// plugin set only.
template <bool EXACT, bool EXT, bool SETS, bool OV = false>
__device__ __forceinline__ uint32_t row_status(const KCfg& cfg, const RowCtx& c, const int64_t* __restrict__ n,
                                               const ZoneRec* __restrict__ zr, uint32_t rec, uint64_t cand,
                                               const Over* ov = nullptr) {
    static_assert(!(EXT && OV), "eval_pair_ext takes its override from the reservation views");
    uint32_t st;
    if constexpr (EXT) st = eval_pair_ext<EXACT>(cfg, *c.e, n, zr, dev_of(*c.e, rec), rec, c.p, c.px, c.q).status;
    else st = eval_pair<EXACT, OV, true, false, false>(cfg, n, zr, c.p, ov).status;
    if constexpr (SETS) st = row_exclude(st, cand, rec);
    return st;
}

}  // namespace kg
#endif
