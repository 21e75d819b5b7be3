// kg_preempt.h — host-side launch interface of the preemption dry run (kg_preempt.hip; internal to libkoordgpu.so) and
// the device form of a snapshot's resident pods.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "../../include/koordgpu.h"
#include "kg_rowfilter.h"

namespace kg {

// Threads of a k_preempt workgroup: one wave, as k_offer_slots (kg_slots.h): the remove / reprieve loop is serial per
// wave and waves share nothing.
// Two forms of the reprieve loop were built. The flat one stepped the whole wave through (group, position) pairs, 1 + 2 x
// the wave's longest list steps, a lane evaluating only in the steps that hit one of its victims; the kept one gives
// every lane its own cursor to its next victim, 1 + the wave's largest victim count steps with every alive lane
// evaluating in each. Measured on one MI355X in separate runs of tools/preempt_rate.py (ms per call to the summaries on
// the host, median of three repeats, flat / cursor; profiles/preempt/preempt_rate_flat_loop.json, preempt_rate.json):
//   10k nodes:   1 preemptor 0.315 / 0.260, 16 preemptors 0.985 / 0.869, 100 preemptors 5.00 / 4.47
//   100k nodes:  1 preemptor 0.586 / 0.540, 16 preemptors 11.5 / 7.1,    100 preemptors 71.0 / 66.0
// From 16 preemptors on most of the call is the copy of the results into memory the caller has just allocated, which
// varies between runs (an earlier run of the cursor form took 10.5 ms where this one took 7.1): the one-preemptor
// figures are the ones that compare the loops.
constexpr uint32_t PREEMPT_WG = 64;
// Record slots a lane keeps in LDS for the loop (the int section and the flag word, odd lane stride): kg_slots.h.
constexpr uint32_t PREEMPT_STAGE = N_FLAGS + 1;
static_assert(PREEMPT_STAGE % 2 == 1, "an odd lane stride in 64-bit words keeps the lanes' LDS reads off one bank");
constexpr uint32_t PREEMPT_MASK_WORDS = KG_RES_MAX_PER_NODE / 32;

// One resident pod as a lane gathers it: 128 bytes, 128-byte aligned, so an entry is one whole cache line and a lane's
// list is consecutive lines (the lanes of a wave read unrelated lists: nothing coalesces across lanes, and a smaller
// entry would share its line with a neighbour the lane reads one iteration later at best). Only this one layout was
// built; no second form was measured.
struct alignas(128) ResEnt {
    int64_t req[5];  // what NodeInfo.RemovePod subtracts: cpu, memory, ephemeral-storage, scalar0, scalar1
    int64_t nz_cpu, nz_mem;
    int64_t start_time;
    int32_t priority, group;
    uint32_t flags;  // KG_RES_*
    int32_t pdb[KG_RES_PDBS];
    uint32_t pad_[11];
};
static_assert(sizeof(ResEnt) == 128, "one cache line per entry");

// The resident table by snapshot position (not by record: kg_snapshot_update_rows moves records, not positions).
// count[i] bit 31 (RES_OVERFLOW): the node's list is longer than KG_RES_MAX_PER_NODE and holds no entries here.
constexpr uint32_t RES_OVERFLOW = 0x80000000u;
struct ResDev {
    const ResEnt* ent;
    const uint32_t* offset;  // [n_nodes] first entry of the node's list, in importance order
    const uint32_t* count;   // [n_nodes]
};

// What the preemptors of one call carry beside their pod rows (device copies, [n_rows]).
struct PreemptRows {
    const int32_t* priority;
    const int32_t* group;        // nullable: every preemptor has group -1
    const int32_t* pdb_allowed;  // [n_pdbs]
    uint32_t n_pdbs;
    uint32_t flags;              // KG_PREEMPT_*
};

// kg_eval_preempt for the n_launch (<= 65535) rows of f from row_base on: out[u * n_nodes + i] of preemptor
// f.rows[row_base + u] on the node at snapshot position i, and (victims non-null) its victim mask at
// victims[(u * n_nodes + i) * PREEMPT_MASK_WORDS]. Every entry of both is written. pr's arrays are the call's, indexed
// by row_base + u. Plain snapshots only (f.ext is refused).
hipError_t launch_preempt(const RowFilter& f, const ResDev& res, const PreemptRows& pr, uint32_t row_base,
                          uint32_t n_launch, kg_preempt_node* out, uint32_t* victims, hipStream_t s);

}  // namespace kg
