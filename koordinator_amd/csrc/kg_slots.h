// kg_slots.h — host-side launch interface of the node offer slot kernel (kg_slots.hip; internal to libkoordgpu.so).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "kg_rowfilter.h"

namespace kg {

// Threads of a k_offer_slots workgroup: one wave. The pod loop is serial per wave and waves share nothing, so small
// workgroups spread a 10k-node snapshot (157 waves) over the compute units instead of packing four waves onto 40.
constexpr uint32_t SLOTS_WG = 64;
// Record slots a lane keeps in LDS for the pod loop: the int section and the flag word, all eval_pair reads of a record
// without its scores. Measured on one MI355X against the form that re-reads the record through cache in every
// iteration (profiles/offer_slots/offer_slots_forms.json; ms per call, cache / LDS, gangs of n copies of one pod):
//   10k nodes:   8 pods 0.063 / 0.060, 64 pods 0.119 / 0.112, 512 pods 0.119 / 0.112
//   100k nodes:  8 pods 0.126 / 0.106, 64 pods 0.352 / 0.229, 512 pods 0.465 / 0.334
// and 4-10 % faster on gangs of distinct pods: staged in all 12 measured cases, so that is the one form kept.
constexpr uint32_t SLOTS_STAGE = N_FLAGS + 1;
static_assert(SLOTS_STAGE % 2 == 1, "an odd lane stride in 64-bit words keeps the lanes' LDS reads off one bank");

// Node offer slots (kg_eval_offer_slots): slots[i], status[i] of the node at snapshot position i for f's rows added
// one after another, network_topology_solver.go:113-158. Every entry of both outputs is written: the caller need not
// clear them. Plain snapshots only (f.ext is refused).
hipError_t launch_offer_slots(const RowFilter& f, uint32_t* slots, uint32_t* status, hipStream_t s);

}  // namespace kg
