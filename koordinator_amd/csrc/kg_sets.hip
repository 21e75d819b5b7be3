// kg_sets.hip — CDNA4 (gfx950) kernels of the per-pod candidate node sets (kg_pods_set_node_sets).
//
//   k_sets_table   the uploaded bitmaps are in snapshot order; select, diagnose and replay walk records in storage-class
//                  order. One wave handles 64 consecutive record positions of one set: each lane reads its record's
//                  snapshot index and that node's bit, the ballot is the set's 64-bit word for those positions.
//   k_select_sets  matrix-mode select of the lanes that carry a set: lane = pod, blockIdx.y = a chunk of records of one
//                  storage class, as k_select. Per 64-record block of the table the lane loads its set's word once; a
//                  block no lane of the wave wants is skipped whole, inside a block a record no lane wants is skipped,
//                  both by wave-uniform branches, so the record index stays a scalar and the record arrives by wide
//                  scalar loads. A pair's bit only masks the insert: the arithmetic is k_select's (fast_eval with the
//                  wave-kind dispatch for waves of fast lanes, their F_BIG records and every record of the other waves on
//                  the integer path, eval_pair). Keys go into the zeroed out rows by atomicMax / the atomic cascade.
//   k_sets_verify  kg_eval_verify's post-pass over its [pod][node] output.
// No MFMA: integer / IEEE-double scalar work, as the other select kernels.
#include <hip/hip_runtime.h>

#include "kg_eval.h"
#include "kg_sets.h"
#include "kg_topk.h"

namespace kg {

// grid (ceil(n_nodes / 256), n_sets): wave w of block x builds word 4 x + w of set y
__global__ __launch_bounds__(256) void k_sets_table(const NodeRec* __restrict__ nodes, uint32_t n_nodes,
                                                    const uint32_t* __restrict__ bits, uint32_t words32, uint32_t words,
                                                    uint64_t* __restrict__ tab) {
    const uint32_t rec = blockIdx.x * 256u + threadIdx.x;
    const uint32_t set = blockIdx.y;
    bool cand = false;
    if (rec < n_nodes) {
        const uint32_t i = node_index(nodes[rec]);  // < n_nodes: the row of the node upload
        cand = (bits[(size_t)set * words32 + (i >> 5)] >> (i & 31u)) & 1u;
    }
    const uint64_t word = __ballot(cand);
    const uint32_t w = rec >> 6;  // uniform over the wave
    if ((threadIdx.x & 63u) == 0u && w < words) tab[(size_t)set * words + w] = word;
}

hipError_t launch_sets_table(const NodeRec* nodes, uint32_t n_nodes, const SetsDev& sd, uint64_t* tab, hipStream_t s) {
    if (n_nodes == 0 || sd.n_sets == 0) return hipSuccess;
    if (sd.n_sets > 65535u) return hipErrorInvalidValue;
    k_sets_table<<<dim3((n_nodes + 255u) / 256u, sd.n_sets), 256, 0, s>>>(nodes, n_nodes, sd.bits, sd.words32, sd.words,
                                                                         tab);
    return hipGetLastError();
}

// the pod is in the float64 fast domain (kg_pods_upload: values below 2^44, no NUMA policy of its own, no cpuset bind)
__device__ __forceinline__ bool sets_lane_fast(const PodV& p) {
    return (p.flags & POD_FASTV) && ((p.flags >> 16) & 15u) == 0u && !(p.flags & KG_POD_CPU_BIND);
}

// The non-F_BIG records of [lo, hi) (lo < hi, one storage class) a lane of the wave wants, on the fast path. srow: the
// lane's row of the record-order table (read by live lanes only). The word index follows i >> 6: chunks begin at any
// record position (class 1 starts where class 0 ends).
template <int K, uint32_t PM, int CLS, int KIND>
__device__ __forceinline__ void sets_fast_loop(const NodeRec* __restrict__ nodes, const ZoneRec* __restrict__ zones,
                                               uint32_t lo, uint32_t hi, uint32_t index_base, const KCfg& cv,
                                               const PodF& pf, const uint64_t* __restrict__ srow, bool live,
                                               uint64_t (&top)[K]) {
    for (uint32_t blk = lo >> 6; blk <= (hi - 1u) >> 6; blk++) {
        const uint64_t word = live ? srow[blk] : 0ull;
        if (!__any(word != 0ull)) continue;  // no lane of the wave has a candidate among these 64 records
        const uint32_t b0 = max(lo, blk << 6), b1 = min(hi, (blk + 1u) << 6);
        for (uint32_t i = b0; i < b1; i++) {
            const bool want = (word >> (i & 63u)) & 1ull;
            if (!__any(want)) continue;
            const FastRec r = *reinterpret_cast<const FastRec*>(&nodes[i].v[FAST_BEGIN]);
            uint32_t total;
            const bool ok = fast_eval<PM, CLS, KIND>(cv, r, zones + i, pf, total);
            const uint64_t key =
                ((uint64_t)total << 32) | (uint64_t)(0xFFFFFFFFu - (index_base + (uint32_t)((uint64_t)r.flags >> 32)));
            // F_BIG records: the integer pass below
            topk_insert<K>(top, (ok & want & !((uint32_t)r.flags & F_BIG)) ? key : 0ull);
        }
    }
}

// grid (lane blocks, nc0 + nc1): block y < nc0 walks class-0 records [y chunk0, ...) of [0, n0), the others class-1
// records of [n0, n_end). FAST: the snapshot allows the fast path; a wave takes it when all its lanes are fast lanes
// (the list is sorted by set, then fast before integer lanes, so few waves mix), else the whole wave runs the integer
// path, which computes the same keys for a fast pod.
template <int K, bool EXACT, bool FAST, uint32_t PM>
__global__ __launch_bounds__(256) void k_select_sets(const NodeRec* __restrict__ nodes, const ZoneRec* __restrict__ zones,
                                                     PodsDev pods, uint32_t n_lanes, const uint32_t* __restrict__ list,
                                                     const int32_t* __restrict__ pod_set,
                                                     const uint64_t* __restrict__ tab, uint32_t words, uint32_t n0,
                                                     uint32_t n_end, uint32_t chunk0, uint32_t chunk1, uint32_t nc0,
                                                     uint32_t index_base, KCfg cfg, uint64_t* __restrict__ out,
                                                     uint32_t* __restrict__ pstat) {
    const GridBlock b = xcd_block();  // whole record chunks per XCD (kg_eval.h)
    const uint32_t j = b.x * blockDim.x + threadIdx.x;
    if ((j & ~63u) >= n_lanes) return;  // a wave past the last lane (no barrier below)
    const bool live = j < n_lanes;
    const uint32_t row = live ? list[j] : 0u;
    const PodV p = load_pod(pods, row);
    const uint64_t* srow = tab + (size_t)(live ? pod_set[row] : 0) * words;  // a listed lane has a set (id >= 0)
    const bool cls1 = b.y >= nc0;  // uniform
    const uint32_t lo = cls1 ? n0 + (b.y - nc0) * chunk1 : b.y * chunk0;
    const uint32_t hi = cls1 ? min(n_end, lo + chunk1) : min(n0, lo + chunk0);
    if (lo >= hi) return;
    uint64_t top[K];
#pragma unroll
    for (int t = 0; t < K; t++) top[t] = 0;
    uint32_t unsup = 0;
    bool wave_fast = false;
    if constexpr (FAST) {
        wave_fast = __all(!live || sets_lane_fast(p));
        if (wave_fast) {
            const PodF pf = to_podf(p, cfg);
            const KCfg cv = cfg_in_vgprs(cfg);
            const bool prod = __all(!live || fast_kind_match(FK_PROD, p)), batch = __all(!live || fast_kind_match(FK_BATCH, p));
            if (!cls1) {
                if (prod) sets_fast_loop<K, PM, 0, FK_PROD>(nodes, zones, lo, hi, index_base, cv, pf, srow, live, top);
                else if (batch) sets_fast_loop<K, PM, 0, FK_BATCH>(nodes, zones, lo, hi, index_base, cv, pf, srow, live, top);
                else sets_fast_loop<K, PM, 0, FK_ANY>(nodes, zones, lo, hi, index_base, cv, pf, srow, live, top);
            } else {
                if (prod) sets_fast_loop<K, PM, 1, FK_PROD>(nodes, zones, lo, hi, index_base, cv, pf, srow, live, top);
                else if (batch) sets_fast_loop<K, PM, 1, FK_BATCH>(nodes, zones, lo, hi, index_base, cv, pf, srow, live, top);
                else sets_fast_loop<K, PM, 1, FK_ANY>(nodes, zones, lo, hi, index_base, cv, pf, srow, live, top);
            }
        }
    }
    // integer pass: the wanted F_BIG records of a fast wave (flagged on the record: lane t looks at record base + t,
    // the ballot is a wave-uniform mask), every wanted record of the other waves
    for (uint32_t blk = lo >> 6; blk <= (hi - 1u) >> 6; blk++) {
        const uint64_t word = live ? srow[blk] : 0ull;
        if (!__any(word != 0ull)) continue;
        const uint32_t base = blk << 6;
        const uint32_t b0 = max(lo, base) - base, b1 = min(hi, base + 64u) - base;  // 0 <= b0 < b1 <= 64
        uint64_t sel = (b1 >= 64u ? ~0ull : (1ull << b1) - 1ull) & ~((1ull << b0) - 1ull);
        if (wave_fast) {
            const uint32_t t = threadIdx.x & 63u;
            bool big = false;
            if (t >= b0 && t < b1) big = ((uint32_t)nodes[base + t].v[N_FLAGS] & F_BIG) != 0;
            sel = __ballot(big);
        }
        while (sel) {
            const uint32_t bit = (uint32_t)__ffsll((unsigned long long)sel) - 1u;
            sel &= sel - 1ull;
            const bool want = (word >> bit) & 1ull;
            if (!__any(want)) continue;
            const uint32_t i = base + bit;
            const PairOut o = eval_pair<EXACT, false, true, true, false>(cfg, nodes[i].v, zones + i, p);
            unsup |= want ? (o.status & KG_ST_UNSUPPORTED) : 0u;
            topk_insert<K>(top, want ? pair_key(cfg, o, rec_gidx(nodes[i], index_base)) : 0ull);
        }
    }
    if (live) {
        if constexpr (K == 1) {
            if (top[0]) atomicMax((unsigned long long*)(out + row), (unsigned long long)top[0]);
        } else {
            topk_atomic<K>(out + (size_t)row * K, top);
        }
        if (unsup) atomicOr(pstat + row, unsup);
    }
}

hipError_t launch_select_sets(const NodeRec* nodes, const ZoneRec* zones, const PodsDev& pods, const uint32_t* list,
                              uint32_t n_lanes, const SetsDev& sd, uint32_t n0, uint32_t n_nodes, uint32_t index_base,
                              uint32_t k, const KCfg& cfg, bool exact, bool fast, uint64_t* out, uint32_t* pstat,
                              hipStream_t s) {
    if (n_lanes == 0 || n_nodes == 0) return hipSuccess;
    if (!list || !sd.pod_set || !sd.tab || sd.words != sets_words(n_nodes) || n0 > n_nodes) return hipErrorInvalidValue;
    // about 2048 workgroups; a chunk is at least one table word long
    const uint32_t lane_blocks = (n_lanes + 255u) / 256u;
    const uint32_t want = max(1u, 2048u / lane_blocks);
    const uint32_t chunk = max(64u, ((n_nodes + want - 1u) / want + 63u) / 64u * 64u);
    const uint32_t nc0 = (n0 + chunk - 1u) / chunk, nc1 = (n_nodes - n0 + chunk - 1u) / chunk;
    if (nc0 + nc1 > 65535u) return hipErrorInvalidValue;
    const dim3 grid(lane_blocks, nc0 + nc1), block(256);
#define KG_SETS_ARGS                                                                                                   \
    nodes, zones, pods, n_lanes, list, sd.pod_set, sd.tab, sd.words, n0, n_nodes, chunk, chunk, nc0, index_base, cfg,  \
        out, pstat
#define KG_SETS_K(EXACTV, FASTV, PMV)                                                                                  \
    do {                                                                                                               \
        if (k == 1) k_select_sets<1, EXACTV, FASTV, PMV><<<grid, block, 0, s>>>(KG_SETS_ARGS);                         \
        else k_select_sets<KG_TOPK_MAX, EXACTV, FASTV, PMV><<<grid, block, 0, s>>>(KG_SETS_ARGS);                      \
    } while (0)
    if (exact) {
        KG_SETS_K(true, false, 0);
    } else if (!fast) {
        KG_SETS_K(false, false, 0);
    } else {
        switch (cfg.plugins & 7u) {
            case 0: KG_SETS_K(false, true, 0); break;
            case 1: KG_SETS_K(false, true, 1); break;
            case 2: KG_SETS_K(false, true, 2); break;
            case 3: KG_SETS_K(false, true, 3); break;
            case 4: KG_SETS_K(false, true, 4); break;
            case 5: KG_SETS_K(false, true, 5); break;
            case 6: KG_SETS_K(false, true, 6); break;
            default: KG_SETS_K(false, true, 7); break;
        }
    }
#undef KG_SETS_K
#undef KG_SETS_ARGS
    return hipGetLastError();
}

// one lane per (pod, node) pair of the verify matrix, in snapshot order like the uploaded bitmap
__global__ __launch_bounds__(256) void k_sets_verify(const int32_t* __restrict__ pod_set,
                                                     const uint32_t* __restrict__ bits, uint32_t words32,
                                                     uint32_t n_pods, uint32_t n_nodes, uint32_t* __restrict__ status,
                                                     int64_t* __restrict__ total) {
    const size_t x = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= (size_t)n_pods * n_nodes) return;
    const uint32_t j = (uint32_t)(x / n_nodes), i = (uint32_t)(x % n_nodes);
    const int32_t set = pod_set[j];
    if (set < 0) return;
    if ((bits[(size_t)set * words32 + (i >> 5)] >> (i & 31u)) & 1u) return;
    status[x] |= KG_ST_NODE_EXCLUDED;
    total[x] = -1;
}

hipError_t launch_sets_verify(const SetsDev& sd, uint32_t n_pods, uint32_t n_nodes, uint32_t* status, int64_t* total,
                              hipStream_t s) {
    const size_t pairs = (size_t)n_pods * n_nodes;
    if (pairs == 0) return hipSuccess;
    k_sets_verify<<<dim3((unsigned)((pairs + 255) / 256)), 256, 0, s>>>(sd.pod_set, sd.bits, sd.words32, n_pods, n_nodes,
                                                                       status, total);
    return hipGetLastError();
}

}  // namespace kg
