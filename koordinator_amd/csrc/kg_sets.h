// kg_sets.h — host-side launch interface of the candidate node set kernels (kg_sets.hip; internal to libkoordgpu.so).
#pragma once
#include <hip/hip_runtime_api.h>

#include "kg_kernels.h"

namespace kg {

// The candidate node sets of a batch on the device (kg_pods_set_node_sets). bits is the uploaded bitmap in snapshot
// order, [set][words32]; tab the same sets in record order for one snapshot layout, [set][words]: bit (r & 63) of
// word (r >> 6) = the node stored at record position r is a candidate.
struct SetsDev {
    const int32_t* pod_set;  // [pod] set id, -1 = none
    const uint32_t* bits;
    const uint64_t* tab;
    uint32_t words32, words, n_sets;
};

inline uint32_t sets_words32(uint32_t n_nodes) { return (n_nodes + 31u) / 32u; }
inline uint32_t sets_words(uint32_t n_nodes) { return (n_nodes + 63u) / 64u; }

// tab[set][r >> 6] from bits[set] and the records' snapshot indices (k_sets_table): every word of every set is written.
hipError_t launch_sets_table(const NodeRec* nodes, uint32_t n_nodes, const SetsDev& sd, uint64_t* tab, hipStream_t s);

// The set lanes of a plain select (k_select_sets): lanes list[0, n_lanes) (pod rows, each with a set), sorted by set;
// keys into the zeroed out[row][K] by atomicMax / the atomic cascade, KG_ST_UNSUPPORTED into pstat[row] by atomicOr.
// fast: the float64 fast path is valid for the snapshot (the lanes' own domain is read from their flags).
hipError_t launch_select_sets(const NodeRec* nodes, const ZoneRec* zones, const PodsDev& pods, const uint32_t* list,
                              uint32_t n_lanes, const SetsDev& sd, uint32_t n0, uint32_t n_nodes, uint32_t index_base,
                              uint32_t k, const KCfg& cfg, bool exact, bool fast, uint64_t* out, uint32_t* pstat,
                              hipStream_t s);

// kg_eval_verify's post-pass over the output matrix ([pod][node], snapshot order): an excluded pair's status takes
// KG_ST_NODE_EXCLUDED and its total -1 (k_sets_verify).
hipError_t launch_sets_verify(const SetsDev& sd, uint32_t n_pods, uint32_t n_nodes, uint32_t* status, int64_t* total,
                              hipStream_t s);

}  // namespace kg
