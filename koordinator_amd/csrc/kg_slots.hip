// kg_slots.hip — CDNA4 (gfx950) kernel of the node offer slots (kg_eval_offer_slots): per node, how many of a job's
// pods fit when they are added one after another (calculateNodeOfferSlot, coscheduling/core/
// network_topology_solver.go:113-158), and the status word of the first pod that does not.
//
// The dependence runs along the pods and nodes are independent, so lane = node record in storage order and the pod row
// is wave-uniform (the pod lives in SGPRs, loaded with scalar loads), k_feasible_by_records' geometry with the pod loop
// inside. What "add" changes is what NodeInfo.AddPodInfo moves (requested cpu / memory / ephemeral-storage / scalars,
// non-zero requested cpu / memory, the pod count): exactly the slots struct Over overrides (kg_eval.h). Each lane keeps
// an Over in registers, seeded from its record, and takes the pair's word against it (row_status with OV,
// kg_rowfilter.h: the filters-only pair evaluation every row-list call shares): the LoadAware bases,
// NUMA zone usage, cpusets stay the snapshot's, as the plugins' AddPod hooks leave them for a pending sibling.
// A lane that failed keeps its word; the wave leaves the loop when no lane is alive. Results go to the node's
// snapshot position: no atomics, no second pass. No MFMA: integer / IEEE-double scalar work.
// The record is read once per lane and kept in LDS for every pod (measured against re-reading it through cache each
// iteration, kg_slots.h); the ZoneRec, which only NUMA nodes read, stays in global memory.
#include <hip/hip_runtime.h>

#include "kg_rowfilter.h"
#include "kg_slots.h"

namespace kg {

// grid ceil(n_nodes / SLOTS_WG) workgroups of one wave. SETS: the pod's set word of the record-order table for the
// wave's 64 records (rec >> 6 is wave-uniform).
template <bool EXACT, bool SETS>
__global__ __launch_bounds__(SLOTS_WG) void k_offer_slots(const NodeRec* __restrict__ nodes,
                                                          const ZoneRec* __restrict__ zones, PodsDev pods,
                                                          const uint32_t* __restrict__ rows, uint32_t n_rows,
                                                          uint32_t n_nodes, KCfg cfg, uint32_t* __restrict__ slots,
                                                          uint32_t* __restrict__ status,
                                                          const int32_t* __restrict__ pod_set,
                                                          const uint64_t* __restrict__ tab, uint32_t words) {
    const uint32_t rec = blockIdx.x * SLOTS_WG + threadIdx.x;
    const bool live = rec < n_nodes;
    const uint32_t r = live ? rec : n_nodes - 1u;  // idle lanes of the last wave read the last record (n_nodes > 0)
    // The slots the Filter reads of a record (the int section and the flag word), staged once per lane in LDS and read
    // from there in every iteration: 16.5 KB per wave. The lane stride is SLOTS_STAGE = 33 slots, an odd number of
    // 64-bit words, so the lanes of a ds_read_b64 pass fall on different bank pairs. Each lane reads only what it
    // wrote: no barrier.
    __shared__ int64_t stage[SLOTS_WG * SLOTS_STAGE];
    for (int q = 0; q < SLOTS_STAGE; q++) stage[threadIdx.x * SLOTS_STAGE + q] = nodes[r].v[q];
    const int64_t* __restrict__ n = stage + threadIdx.x * SLOTS_STAGE;
    const ZoneRec* __restrict__ zr = zones + r;
    Over ov;
    ov.req[0] = n[N_REQ_CPU];
    ov.req[1] = n[N_REQ_MEM];
    ov.req[2] = n[N_REQ_EPH];
    ov.req[3] = n[N_SC_REQ0];
    ov.req[4] = n[N_SC_REQ1];
    ov.nz_cpu = n[N_NZ_CPU];
    ov.nz_mem = n[N_NZ_MEM];
    ov.num_pods = n[N_NUM_PODS];
    bool alive = live;
    uint32_t slot = 0u, word = 0u;
    for (uint32_t t = 0; t < n_rows; t++) {
        if (!__any(alive)) break;  // uniform
        const uint32_t j = __builtin_amdgcn_readfirstlane(rows ? rows[t] : t);
        const RowCtx c = row_ctx<false>(pods, j, true, nullptr, nullptr);
        const PodV& p = c.p;
        const uint64_t cand = row_cand(row_set<SETS>(pod_set, tab, words, j), r);
        if (alive) {
            const uint32_t st = row_status<EXACT, false, SETS, true>(cfg, c, n, zr, r, cand, &ov);
            if (st) {
                word = st;
                alive = false;
            } else {  // NodeInfo.AddPodInfo
                ov.req[0] += p.req_cpu;
                ov.req[1] += p.req_mem;
                ov.req[2] += p.req_eph;
                ov.req[3] += p.sc0;
                ov.req[4] += p.sc1;
                ov.nz_cpu += p.nz_cpu;
                ov.nz_mem += p.nz_mem;
                ov.num_pods += 1;
                slot++;
            }
        }
    }
    if (live) {
        const uint32_t i = node_index(nodes[rec]);  // < n_nodes
        slots[i] = slot;
        status[i] = word;
    }
}

hipError_t launch_offer_slots(const RowFilter& f, uint32_t* slots, uint32_t* status, hipStream_t s) {
    if (f.n_nodes == 0) return hipSuccess;
    if (!rowfilter_valid(f) || f.ext || !slots || !status) return hipErrorInvalidValue;
    const uint32_t grid = (f.n_nodes + SLOTS_WG - 1u) / SLOTS_WG;
    rowfilter_dispatch<false>(f, [&](auto exact, auto, auto sets) {
        k_offer_slots<decltype(exact)::value, decltype(sets)::value><<<grid, SLOTS_WG, 0, s>>>(
            f.nodes, f.zones, f.pods, f.rows, f.n_rows, f.n_nodes, f.cfg, slots, status, f.pod_set, f.tab,
            sets_words(f.n_nodes));
    });
    return hipGetLastError();
}

}  // namespace kg
