// kg_diag.h — host-side launch interface of the FitError diagnosis kernels (kg_diag.hip; internal to libkoordgpu.so).
#pragma once
#include <hip/hip_runtime_api.h>

#include "kg_rowfilter.h"

namespace kg {

// Records one lane may walk per launch of the diagnosis loop: its counters are packed 8-bit fields (kg_diag.hip).
constexpr uint32_t DIAG_MAX_CHUNK = 255;
// Shortest chunk the launcher cuts (a one-pod request over 100k nodes still spreads over the chip).
constexpr uint32_t DIAG_MIN_CHUNK = 32;
// Workgroups the launcher aims for (256 compute units, several waves each).
constexpr uint32_t DIAG_TARGET_BLOCKS = 2048;

// Chunk length for n_rows requested rows over n_nodes records: ceil(n_nodes / chunks) with enough chunks to reach
// `target` workgroups, never above DIAG_MAX_CHUNK and not below DIAG_MIN_CHUNK.
inline uint32_t diag_chunk(uint32_t n_nodes, uint32_t n_rows, uint32_t block, uint32_t target = DIAG_TARGET_BLOCKS) {
    const uint32_t row_blocks = (n_rows + block - 1) / block;
    const uint32_t want = row_blocks ? (target + row_blocks - 1) / row_blocks : 1u;
    uint32_t chunk = (n_nodes + want - 1) / (want ? want : 1u);
    if (chunk < DIAG_MIN_CHUNK) chunk = DIAG_MIN_CHUNK;
    if (chunk > DIAG_MAX_CHUNK) chunk = DIAG_MAX_CHUNK;
    return chunk;
}

// Reason node counts of the requested rows (kg_eval_diagnose): counts[t][KG_DIAG_SLOTS] += the histogram of the
// counted status words of f's row t over every record. counts must be zeroed by the caller (on the same stream);
// first_plugin: KG_DIAG_FIRST_PLUGIN.
hipError_t launch_diagnose(const RowFilter& f, bool first_plugin, uint32_t* counts, hipStream_t s);

}  // namespace kg
