// kg_feasible.h — host-side launch interface of the feasible-node bitmap kernels (kg_feasible.hip; internal to
// libkoordgpu.so). The geometry helpers are plain C++: tests/native/feasible_geom_main.cpp compiles them on the host.
#pragma once
#include <cstdint>

namespace kg {

// Step 1 has two forms (kg_feasible.hip): lane = row (k_feasible_by_rows) and lane = record (k_feasible_by_records).
// Measured on one MI355X (tools/feasible_rate.py, profiles/feasible/feasible_rate.json and
// feasible_rate_breakeven.json; ms per call, rows form / records form): the break-even is not one row count, it
// follows the pair count.
//   10k nodes:   1 row 0.158 / 0.040, 100 rows 0.173 / 0.077, 400 rows (4.0M pairs) 0.207 / 0.181, 1000 rows (10M pairs)
//                0.276 / 0.394, 10000 rows 2.09 / 3.41
//   100k nodes:  1 row 0.148 / 0.043, 16 rows (1.6M pairs) 0.247 / 0.189, 32 rows (3.2M pairs) 0.256 / 0.329, 64 rows
//                0.287 / 0.611, 10000 rows 28.9 / 87.6
// The rows form costs 0.15 ms at the least (a lane walks 64 records or more one after the other), the records form
// 0.04 ms and then 0.03-0.09 ms per million pairs. The rows form runs from FEAS_PAIRS_MIN pairs on, given at least
// FEAS_ROWS_MIN rows (the fewest at which it was seen to win: half a wave of live lanes); of the 20 measured cases only
// 400 rows x 10k nodes then takes the slower form, by 0.026 ms.
constexpr uint64_t FEAS_PAIRS_MIN = 3000000;
constexpr uint32_t FEAS_ROWS_MIN = 32;
inline bool feasible_rows_form(uint32_t n_rows, uint32_t n_nodes) {
    return n_rows >= FEAS_ROWS_MIN && (uint64_t)n_rows * n_nodes >= FEAS_PAIRS_MIN;
}
// Workgroups the lane = row form aims for (256 compute units, several waves each), as DIAG_TARGET_BLOCKS.
constexpr uint32_t FEAS_TARGET_BLOCKS = 2048;
// Rows one workgroup of step 2 (k_feasible_rows) serves with one load of its 256 record positions.
constexpr uint32_t FEAS_ROWS_PER_BLOCK = 8;
// gridDim.y of a launch; larger requests take several launches.
constexpr uint32_t FEAS_MAX_Y = 65535;

inline uint32_t feasible_words32(uint32_t n_nodes) { return (n_nodes + 31u) / 32u; }  // output words of one row
inline uint32_t feasible_words(uint32_t n_nodes) { return (n_nodes + 63u) / 64u; }    // record-order words of one row

// Chunk length of the lane = row form for n_rows requested rows over n_nodes records: ceil(n_nodes / chunks) with
// enough chunks to reach `target` workgroups, rounded up to whole 64-record words and never below one. Chunk y starts
// at record y * chunk, a multiple of 64: every word of the record-order bitmap has one writer.
inline uint32_t feasible_chunk(uint32_t n_nodes, uint32_t n_rows, uint32_t block, uint32_t target = FEAS_TARGET_BLOCKS) {
    const uint32_t row_blocks = block ? (n_rows + block - 1u) / block : 0u;
    const uint32_t want = row_blocks ? (target + row_blocks - 1u) / row_blocks : 1u;
    const uint32_t len = (n_nodes + (want ? want : 1u) - 1u) / (want ? want : 1u);
    const uint32_t chunk = (len + 63u) / 64u * 64u;
    return chunk ? chunk : 64u;
}

// Records one launch of the lane = row form covers: FEAS_MAX_Y chunks (a multiple of 64 records as well).
inline uint64_t feasible_span(uint32_t chunk) { return (uint64_t)FEAS_MAX_Y * chunk; }

}  // namespace kg

#ifndef KG_FEASIBLE_GEOMETRY_ONLY  // the stand-alone host test takes the helpers above only
#include <hip/hip_runtime_api.h>

#include "kg_rowfilter.h"

namespace kg {

// Step 1 (kg_eval_feasible): rtab[t][w], w < feasible_words(n_nodes): bit (r & 63) of word (r >> 6) = the status word
// of (f's row t, the node stored at record position r) has no bit of fail_mask; bits at or above n_nodes are 0. Every
// word is written: the caller need not clear rtab. The form follows feasible_rows_form, or
// KG_FEASIBLE_FORM=rows|records (read per call).
hipError_t launch_feasible_records(const RowFilter& f, uint32_t fail_mask, uint64_t* rtab, hipStream_t s);

// Step 2: out[t][w], w < feasible_words32(n_nodes): bit (i & 31) of word (i >> 5) = rtab[t]'s bit of record position
// pos[i] (the snapshot index -> record position map); bits at or above n_nodes are 0. count (nullable, zeroed by the
// caller on the same stream): count[t] += the row's population count.
hipError_t launch_feasible_rows(const uint64_t* rtab, const uint32_t* pos, uint32_t n_rows, uint32_t n_nodes,
                                uint32_t* out, uint32_t* count, hipStream_t s);

}  // namespace kg
#endif
