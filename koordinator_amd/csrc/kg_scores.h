// kg_scores.h — host-side launch interface of the host score term kernels (kg_scores.hip; internal to libkoordgpu.so).
#pragma once
#include <hip/hip_runtime_api.h>

#include "kg_kernels.h"

namespace kg {

// The host score terms of a batch on the device (kg_pods_set_node_scores). raw is the uploaded rows in snapshot order,
// [row][n_nodes]; rtab the same rows in record order for one snapshot layout: rtab[row][r] = raw[row][snapshot index of
// the node stored at record position r].
struct ScoresDev {
    const int32_t* pod_terms;  // [pod][KG_SCORE_TERMS] row id, -1 = unused slot
    const int32_t* raw;
    const int32_t* rtab;
    const uint32_t* mode;    // [row] KG_SCORE_*
    const uint32_t* weight;  // [row]
    uint32_t n_rows, n_nodes;
};

// One term's value on a feasible candidate: raw, or DefaultNormalizeScore(100, reverse) of raw against m, the largest
// raw over the pod's feasible candidates (frameworkext/normalize_score.go:24-52; integer division). raw <= m.
KG_HD inline uint32_t score_term_value(uint32_t mode, uint32_t raw, uint32_t m) {
    if (mode == KG_SCORE_RAW) return raw;
    if (m == 0) return mode == KG_SCORE_NORMALIZE_REVERSE ? 100u : 0u;
    const uint32_t q = 100u * raw / m;
    return mode == KG_SCORE_NORMALIZE_REVERSE ? 100u - q : q;
}

// rtab from raw and the records' snapshot indices (k_scores_table): every entry of every row is written.
hipError_t launch_scores_table(const NodeRec* nodes, uint32_t n_nodes, const ScoresDev& sd, int32_t* rtab, hipStream_t s);

// The term lanes of a plain select (k_select_scores): lanes list[0, n_lanes) (pod rows, each with a term; pod_set /
// tab / words: their candidate node sets as SetsDev has them, pod_set == nullptr: the batch carries none), sorted by
// (set, term tuple). lmax: [n_lanes][KG_SCORE_TERMS] scratch, zeroed here. norm: some listed lane has a normalised term
// (pass 1 runs). Keys into the zeroed out[row][K] by atomicMax / the atomic cascade, KG_ST_UNSUPPORTED into pstat[row]
// by atomicOr. fast: the float64 fast path is valid for the snapshot.
hipError_t launch_select_scores(const NodeRec* nodes, const ZoneRec* zones, const PodsDev& pods, const uint32_t* list,
                                uint32_t n_lanes, const int32_t* pod_set, const uint64_t* tab, uint32_t words,
                                const ScoresDev& sd, uint32_t* lmax, bool norm, uint32_t n0, uint32_t n_nodes,
                                uint32_t index_base, uint32_t k, const KCfg& cfg, bool exact, bool fast, uint64_t* out,
                                uint32_t* pstat, hipStream_t s);

// kg_eval_verify's post-pass over the output matrix ([pod][node], snapshot order), after the sets' one: per pod row the
// maxima over the pairs with status 0, then total += sum of weight x value on those pairs (k_scores_verify).
hipError_t launch_scores_verify(const ScoresDev& sd, uint32_t n_pods, uint32_t n_nodes, const uint32_t* status,
                                int64_t* total, hipStream_t s);

}  // namespace kg
