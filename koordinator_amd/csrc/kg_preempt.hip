// kg_preempt.hip — CDNA4 (gfx950) kernel of the preemption dry run (kg_eval_preempt): SelectVictimsOnNode
// (elasticquota/preempt.go:111-217, reservation/preemption.go:123-219) of one preemptor on every node of a snapshot.
//
// Nodes are independent and the dependence runs along a node's resident pods, so the geometry is k_offer_slots'
// (kg_slots.hip): one-wave workgroups, lane = node record in storage order, blockIdx.y = the preemptor's row, the pod
// wave-uniform, the record's Filter slots staged once per lane in LDS with the odd lane stride. What removing and adding
// back a resident pod changes is what NodeInfo.RemovePod / AddPodInfo move, the slots of struct Over (kg_eval.h); the
// pair's word against it is row_status with OV (kg_rowfilter.h). The LoadAware bases, NUMA zone usage and cpusets stay
// the snapshot's: LoadAware has no AddPod / RemovePod hook, and a victim that holds a NUMA / cpuset allocation is
// refused per node (KG_PREEMPT_UNSUPPORTED) instead of followed.
//
// A lane walks its node's list (ResEnt, one cache line per entry, importance order) twice:
//   pass 1  marks the potential victims, removes them from the Over and splits them by PodDisruptionBudget. The split
//           wants a per-node copy of the allowed counts; a lane has no room for n_pdbs counters, so an entry that names
//           a budget counts the potential victims up to itself that name it too (a rescan of the lines it has just
//           read: few entries name a budget) and is violating when that count exceeds the allowed one.
//   pass 2  is one loop with one Filter call site: step 0 takes the word with every potential victim removed; in the
//           steps after it each lane adds back its next victim (the violating ones from the most important, then the
//           others) and takes the word (non-zero: removed again, a victim).
// Per-lane list lengths differ: the wave loops to its longest list and leaves when no lane is alive. The two
// per-position bit masks (victim, violating) live in LDS, word-major so the lanes of a wave fall on different banks; the
// owning lane stores its node's result and victim mask with plain vector stores. No atomics, no MFMA.
#include <hip/hip_runtime.h>

#include "kg_preempt.h"
#include "kg_rowfilter.h"

namespace kg {

namespace {

constexpr int M_VICTIM = 0, M_VIOLATING = 1;

struct Masks {
    uint32_t* w;  // [2][PREEMPT_MASK_WORDS][PREEMPT_WG] of the workgroup, this lane's column
    __device__ __forceinline__ uint32_t& at(int m, uint32_t k) { return w[(m * PREEMPT_MASK_WORDS + (k >> 5)) * PREEMPT_WG]; }
    __device__ __forceinline__ bool get(int m, uint32_t k) { return (at(m, k) >> (k & 31u)) & 1u; }
    __device__ __forceinline__ void set(int m, uint32_t k) { at(m, k) |= 1u << (k & 31u); }
    __device__ __forceinline__ void clear(int m, uint32_t k) { at(m, k) &= ~(1u << (k & 31u)); }
    // The first victim position >= k (< cnt) of group g (0: violating, 1: the others), or cnt.
    __device__ __forceinline__ uint32_t next(uint32_t g, uint32_t k, uint32_t cnt) {
        while (k < cnt) {
            const uint32_t viol = at(M_VIOLATING, k);
            const uint32_t bits = (at(M_VICTIM, k) & (g == 0u ? viol : ~viol)) >> (k & 31u);
            if (bits) return min(k + (uint32_t)__ffs((int)bits) - 1u, cnt);
            k = (k | 31u) + 1u;
        }
        return cnt;
    }
};

__device__ __forceinline__ void over_move(Over& ov, const ResEnt& e, int64_t sign) {
#pragma unroll
    for (int q = 0; q < 5; q++) ov.req[q] += sign * e.req[q];
    ov.nz_cpu += sign * e.nz_cpu;
    ov.nz_mem += sign * e.nz_mem;
    ov.num_pods += sign;
}

}  // namespace

// grid (ceil(n_nodes / PREEMPT_WG), rows of this launch) workgroups of one wave; row_base: the first of them in the
// call's row list (the outputs are the launch's own).
template <bool EXACT, bool SETS>
__global__ __launch_bounds__(PREEMPT_WG) void k_preempt(const NodeRec* __restrict__ nodes,
                                                        const ZoneRec* __restrict__ zones, PodsDev pods,
                                                        const uint32_t* __restrict__ rows, uint32_t row_base,
                                                        uint32_t n_nodes, KCfg cfg, ResDev res, PreemptRows pr,
                                                        kg_preempt_node* __restrict__ out,
                                                        uint32_t* __restrict__ victims,
                                                        const int32_t* __restrict__ pod_set,
                                                        const uint64_t* __restrict__ tab, uint32_t words) {
    const uint32_t rec = blockIdx.x * PREEMPT_WG + threadIdx.x;
    const bool live = rec < n_nodes;
    const uint32_t r = live ? rec : n_nodes - 1u;  // idle lanes of the last wave read the last record (n_nodes > 0)
    __shared__ int64_t stage[PREEMPT_WG * PREEMPT_STAGE];
    __shared__ uint32_t mask_words[2 * PREEMPT_MASK_WORDS * PREEMPT_WG];
    for (int q = 0; q < (int)PREEMPT_STAGE; q++) stage[threadIdx.x * PREEMPT_STAGE + q] = nodes[r].v[q];
    const int64_t* __restrict__ n = stage + threadIdx.x * PREEMPT_STAGE;
    const ZoneRec* __restrict__ zr = zones + r;
    Masks mk{mask_words + threadIdx.x};
    for (uint32_t k = 0; k < KG_RES_MAX_PER_NODE; k += 32) mk.at(M_VICTIM, k) = mk.at(M_VIOLATING, k) = 0u;

    const uint32_t t = row_base + blockIdx.y;
    const uint32_t j = __builtin_amdgcn_readfirstlane(rows ? rows[t] : t);
    const int32_t prio = pr.priority[t];
    const int32_t group = pr.group ? pr.group[t] : -1;
    const RowCtx c = row_ctx<false>(pods, j, true, nullptr, nullptr);
    const bool numa_follows = (cfg.plugins & KG_PLUGIN_NUMA) && !(c.p.flags & KG_POD_NUMA_SKIP);
    const RowSet rs = row_set<SETS>(pod_set, tab, words, j);
    const bool excluded = SETS && !((row_cand(rs, r) >> (r & 63u)) & 1ull);

    const uint32_t i = (uint32_t)((uint64_t)n[N_FLAGS] >> 32);  // the node's snapshot position, < n_nodes
    const uint32_t cw = res.count[i];
    const bool overflow = (cw & RES_OVERFLOW) != 0;
    const uint32_t cnt = (live && !excluded && !overflow) ? cw : 0u;  // <= KG_RES_MAX_PER_NODE (the upload's rule)
    const ResEnt* __restrict__ ent = res.ent + res.offset[i];

    Over ov;
    ov.req[0] = n[N_REQ_CPU];
    ov.req[1] = n[N_REQ_MEM];
    ov.req[2] = n[N_REQ_EPH];
    ov.req[3] = n[N_SC_REQ0];
    ov.req[4] = n[N_SC_REQ1];
    ov.nz_cpu = n[N_NZ_CPU];
    ov.nz_mem = n[N_NZ_MEM];
    ov.num_pods = n[N_NUM_PODS];

    // ---- pass 1: potential victims, removed; the PDB split ------------------------------------------------------
    uint32_t n_pot = 0;
    bool refused = overflow;
    for (uint32_t k = 0; __any(k < cnt); k++) {
        if (k >= cnt) continue;
        const ResEnt& e = ent[k];
        const uint32_t ef = e.flags;
        bool pot = e.priority < prio;
        if ((pr.flags & KG_PREEMPT_SKIP_NON_PREEMPTIBLE) && (ef & KG_RES_NON_PREEMPTIBLE)) pot = false;
        if ((pr.flags & KG_PREEMPT_SAME_GROUP) && e.group != group) pot = false;
        if (!pot) continue;
        mk.set(M_VICTIM, k);
        n_pot++;
        over_move(ov, e, -1);
        if ((ef & KG_RES_PDB_OVERFLOW) || ((ef & KG_RES_NUMA_ALLOC) && numa_follows)) refused = true;
        bool viol = false;
        for (int b = 0; b < KG_RES_PDBS; b++) {
            const int32_t id = e.pdb[b];  // < n_pdbs (checked by the host before the launch)
            if (id < 0) continue;
            int32_t used = 0;  // the decrements of budget id by the potential victims up to this one
            for (uint32_t q = 0; q <= k; q++) {
                if (!mk.get(M_VICTIM, q)) continue;
                for (int b2 = 0; b2 < KG_RES_PDBS; b2++) used += ent[q].pdb[b2] == id;
            }
            viol |= pr.pdb_allowed[id] - used < 0;
        }
        if (viol) mk.set(M_VIOLATING, k);
    }

    // ---- pass 2: the word with all of them removed, then the reprieve --------------------------------------------
    // Step 0 takes the removal word. After it every alive lane moves its own cursor (group g, position k) to its next
    // victim of the group, so each step evaluates one add-back on every alive lane: the wave runs 1 + its largest number
    // of potential victims steps, not twice its longest list.
    bool alive = live && !excluded && !refused && n_pot > 0;
    uint32_t word = 0u, n_vic = 0u, n_vviol = 0u;
    int32_t top_prio = 0;
    int64_t sum_prio = 0, top_start = 0;
    uint8_t result = KG_PREEMPT_CANDIDATE;
    uint32_t g = 0u, k = 0u;  // 0: the violating group
    for (bool first = true; __any(alive); first = false) {
        if (!alive) continue;
        if (!first) {
            k = mk.next(g, k, cnt);
            if (k >= cnt && g == 0u) {
                g = 1u;
                k = mk.next(g, 0u, cnt);
            }
            if (k >= cnt) {  // every potential victim had its turn
                alive = false;
                continue;
            }
        }
        const ResEnt& e = ent[k];  // read in the add-back steps only
        if (!first) over_move(ov, e, 1);
        const uint32_t st = row_status<EXACT, false, false, true>(cfg, c, n, zr, r, ~0ull, &ov);
        if (st & KG_ST_UNSUPPORTED) {
            result = KG_PREEMPT_UNSUPPORTED;
            word = st;
            alive = false;
        } else if (first) {
            if (st) {
                result = KG_PREEMPT_NO_FIT;
                word = st;
                alive = false;
            }
        } else {
            if (st == 0u) {
                mk.clear(M_VICTIM, k);  // reprieved: the pod stays
            } else {
                over_move(ov, e, -1);  // removed again: a victim
                const int32_t ep = e.priority;
                const int64_t es = e.start_time;
                if (n_vic == 0u || ep > top_prio || (ep == top_prio && es < top_start)) {
                    top_prio = ep;
                    top_start = es;
                }
                sum_prio += ep;
                n_vic++;
                n_vviol += g == 0u;
            }
            k++;
        }
    }

    if (!live) return;
    if (excluded) {
        result = KG_PREEMPT_EXCLUDED;
        word = KG_ST_NODE_EXCLUDED;
    } else if (overflow) {
        result = KG_PREEMPT_UNSUPPORTED;
        word = KG_ST_UNSUPPORTED;
    } else if (n_pot == 0u) {
        result = KG_PREEMPT_NO_VICTIMS;
    } else if (refused) {
        result = KG_PREEMPT_UNSUPPORTED;
        word = KG_ST_UNSUPPORTED;
    }
    if (result != KG_PREEMPT_CANDIDATE) n_vic = n_vviol = 0u, top_prio = 0, sum_prio = 0, top_start = 0;
    kg_preempt_node o;
    o.status = word;
    o.result = result;
    o.pad_ = 0;
    o.n_victims = (uint16_t)n_vic;
    o.n_violating = (uint16_t)n_vviol;
    o.n_potential = (uint16_t)n_pot;  // 0 where nothing was evaluated
    o.top_priority = top_prio;
    o.sum_priority = sum_prio;
    o.top_start = top_start;
    const size_t y = (size_t)blockIdx.y * n_nodes + i;
    out[y] = o;
    if (victims)
        for (uint32_t k = 0; k < KG_RES_MAX_PER_NODE; k += 32)
            victims[y * PREEMPT_MASK_WORDS + (k >> 5)] = result == KG_PREEMPT_CANDIDATE ? mk.at(M_VICTIM, k) : 0u;
}

hipError_t launch_preempt(const RowFilter& f, const ResDev& res, const PreemptRows& pr, uint32_t row_base,
                          uint32_t n_launch, kg_preempt_node* out, uint32_t* victims, hipStream_t s) {
    if (f.n_nodes == 0 || n_launch == 0) return hipSuccess;
    if (n_launch > 65535u || row_base + n_launch > f.n_rows) return hipErrorInvalidValue;
    if (!rowfilter_valid(f) || f.ext || !out || !res.ent || !res.offset || !res.count || !pr.priority ||
        (pr.n_pdbs && !pr.pdb_allowed))
        return hipErrorInvalidValue;
    const dim3 grid((f.n_nodes + PREEMPT_WG - 1u) / PREEMPT_WG, n_launch);
    rowfilter_dispatch<false>(f, [&](auto exact, auto, auto sets) {
        k_preempt<decltype(exact)::value, decltype(sets)::value><<<grid, PREEMPT_WG, 0, s>>>(
            f.nodes, f.zones, f.pods, f.rows, row_base, f.n_nodes, f.cfg, res, pr, out, victims, f.pod_set, f.tab,
            sets_words(f.n_nodes));
    });
    return hipGetLastError();
}

}  // namespace kg
