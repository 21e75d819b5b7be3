// kg_scores.hip — CDNA4 (gfx950) kernels of the per-pod host score terms (kg_pods_set_node_scores).
//
//   k_scores_table   the uploaded raw rows are in snapshot order; the select walks records in storage-class order. One
//                    lane per (row, record position): it reads its record's snapshot index and gathers.
//   k_select_scores  matrix-mode select of the lanes that carry a term: lane = pod, blockIdx.y = a chunk of records of
//                    one storage class, as k_select_sets, whose walk this is (a lane without a candidate node set wants
//                    every record). The arithmetic of a pair is k_select's (fast_eval with the wave-kind dispatch for
//                    waves of fast lanes, their F_BIG records and every record of the other waves on the integer path,
//                    eval_pair). PASS 1 (only waves with a normalised term): the largest raw of each term over the
//                    lane's feasible candidates, atomicMax into the zeroed lmax[lane][term]. PASS 2: the same walk,
//                    the key's total is koord's plus the sum of weight x value; keys go into the zeroed out rows by
//                    atomicMax / the atomic cascade. A wave whose live lanes all name the same row in every slot (the
//                    lanes are sorted by term tuple) reads the raw values through the scalar path (row and record
//                    index are both wave-uniform) in a loop instantiated for that; the other waves by one 4-byte load
//                    per lane and term.
//   k_scores_verify  kg_eval_verify's post-pass over its [pod][node] output, one workgroup per pod row.
// No MFMA: integer / IEEE-double scalar work, as the other select kernels.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "kg_eval.h"
#include "kg_scores.h"
#include "kg_topk.h"

namespace kg {

constexpr int ST = KG_SCORE_TERMS;

// grid (ceil(n_nodes / 256), n_rows)
__global__ __launch_bounds__(256) void k_scores_table(const NodeRec* __restrict__ nodes, uint32_t n_nodes,
                                                      const int32_t* __restrict__ raw, int32_t* __restrict__ rtab) {
    const uint32_t rec = blockIdx.x * 256u + threadIdx.x;
    if (rec >= n_nodes) return;
    const uint32_t i = node_index(nodes[rec]);  // < n_nodes: the row of the node upload
    rtab[(size_t)blockIdx.y * n_nodes + rec] = raw[(size_t)blockIdx.y * n_nodes + i];
}

hipError_t launch_scores_table(const NodeRec* nodes, uint32_t n_nodes, const ScoresDev& sd, int32_t* rtab, hipStream_t s) {
    if (n_nodes == 0 || sd.n_rows == 0) return hipSuccess;
    if (sd.n_rows > 65535u || sd.n_nodes != n_nodes) return hipErrorInvalidValue;
    k_scores_table<<<dim3((n_nodes + 255u) / 256u, sd.n_rows), 256, 0, s>>>(nodes, n_nodes, sd.raw, rtab);
    return hipGetLastError();
}

// the pod is in the float64 fast domain (kg_pods_upload: values below 2^44, no NUMA policy of its own, no cpuset bind)
__device__ __forceinline__ bool scores_lane_fast(const PodV& p) {
    return (p.flags & POD_FASTV) && ((p.flags >> 16) & 15u) == 0u && !(p.flags & KG_POD_CPU_BIND);
}

// The terms of one wave. Per lane: the row, mode and weight of each slot (an unused slot and a dead lane: row -1,
// weight 0, RAW). Per wave, decided once: used = some live lane has a row in the slot; uni = every live lane has the
// same row there (s_row, through readfirstlane: lane 0 of a launched wave is live), so that row's values arrive by
// scalar loads; norm = some live lane's slot is normalised.
struct WaveTerms {
    int32_t row[ST];
    uint32_t mode[ST], weight[ST];
    int32_t s_row[ST];
    bool used[ST], uni[ST], norm[ST];
};

__device__ __forceinline__ WaveTerms load_terms(const ScoresDev& sd, uint32_t pod, bool live) {
    WaveTerms w;
#pragma unroll
    for (int t = 0; t < ST; t++) {
        const int32_t r = live ? sd.pod_terms[(size_t)pod * ST + t] : -1;
        w.row[t] = r;
        w.mode[t] = r >= 0 ? sd.mode[r] : KG_SCORE_RAW;
        w.weight[t] = r >= 0 ? sd.weight[r] : 0u;
        w.s_row[t] = __builtin_amdgcn_readfirstlane(r);
        w.used[t] = __any(r >= 0);
        w.uni[t] = __all(!live || r == w.s_row[t]);
        w.norm[t] = __any(w.mode[t] != KG_SCORE_RAW);
    }
    return w;
}

// Raw value of a used slot t at record position i (wave-uniform). UNI: every used slot of the wave is uniform, the
// address is made of s_row and i alone and the value arrives by a scalar load. Else one 4-byte load per lane, 0 for a
// lane without a row there. UNI is a template parameter and not a branch on w.uni[t]: with both loads in one function
// the compiler merges them into the per-lane form (select of the addresses, one global_load_dword).
template <bool UNI>
__device__ __forceinline__ uint32_t term_raw(const WaveTerms& w, int t, const int32_t* __restrict__ rtab, uint32_t n_nodes,
                                             uint32_t i) {
    if constexpr (UNI) return (uint32_t)rtab[(size_t)(uint32_t)w.s_row[t] * n_nodes + i];  // used and uniform: s_row >= 0
    else return w.row[t] >= 0 ? (uint32_t)rtab[(size_t)(uint32_t)w.row[t] * n_nodes + i] : 0u;
}

__device__ __forceinline__ bool terms_all_uniform(const WaveTerms& w) {
    bool u = true;
#pragma unroll
    for (int t = 0; t < ST; t++) u &= !w.used[t] || w.uni[t];
    return u;
}

// floor(x / m) for m >= 1 and x <= 100 m (x = 100 raw of a feasible candidate, raw <= m <= 2^20), rcp = 1.0f / m: the
// float product is within 2^-22 of the quotient relatively, so below 1 absolutely, and one step either way corrects it.
__device__ __forceinline__ uint32_t div_small(uint32_t x, uint32_t m, float rcp) {
    uint32_t q = (uint32_t)((float)x * rcp);
    const int32_t rem = (int32_t)(x - q * m);
    q -= rem < 0 ? 1u : 0u;
    q += rem >= (int32_t)m ? 1u : 0u;
    return q;
}

// sum over the slots of weight x value on a feasible candidate (mx: the lane's pass-1 maxima, rcp their reciprocals)
template <bool UNI>
__device__ __forceinline__ uint32_t terms_add(const WaveTerms& w, const uint32_t (&mx)[ST], const float (&rcp)[ST],
                                              const int32_t* __restrict__ rtab, uint32_t n_nodes, uint32_t i) {
    uint32_t add = 0;
#pragma unroll
    for (int t = 0; t < ST; t++) {
        if (!w.used[t]) continue;  // wave-uniform
        const uint32_t raw = term_raw<UNI>(w, t, rtab, n_nodes, i);
        uint32_t val = raw;
        if (w.norm[t]) {  // wave-uniform
            const bool rev = w.mode[t] == KG_SCORE_NORMALIZE_REVERSE;
            const uint32_t q = div_small(100u * raw, max(mx[t], 1u), rcp[t]);
            const uint32_t nv = mx[t] == 0u ? (rev ? 100u : 0u) : (rev ? 100u - q : q);
            val = w.mode[t] == KG_SCORE_RAW ? raw : nv;
        }
        add += w.weight[t] * val;
    }
    return add;
}

// The non-F_BIG records of [lo, hi) (lo < hi, one storage class) a lane of the wave wants, on the fast path, as
// sets_fast_loop walks them. srow: the lane's row of the candidate-set table, nullptr = every record. visit(i, ok,
// total, gidx, uni): i wave-uniform; ok = the pair is a feasible candidate of this lane; uni = std::bool_constant<UNI>,
// the load form of the raw values (term_raw).
template <uint32_t PM, int CLS, int KIND, bool UNI, class F>
__device__ __forceinline__ void scores_fast_loop(const NodeRec* __restrict__ nodes, const ZoneRec* __restrict__ zones,
                                                 uint32_t lo, uint32_t hi, uint32_t index_base, const KCfg& cv,
                                                 const PodF& pf, const uint64_t* __restrict__ srow, bool live, F&& visit) {
    for (uint32_t blk = lo >> 6; blk <= (hi - 1u) >> 6; blk++) {
        const uint64_t word = live ? (srow ? srow[blk] : ~0ull) : 0ull;
        if (!__any(word != 0ull)) continue;
        const uint32_t b0 = max(lo, blk << 6), b1 = min(hi, (blk + 1u) << 6);
        for (uint32_t i = b0; i < b1; i++) {
            const bool want = (word >> (i & 63u)) & 1ull;
            if (!__any(want)) continue;
            const FastRec r = *reinterpret_cast<const FastRec*>(&nodes[i].v[FAST_BEGIN]);
            uint32_t total;
            const bool ok = fast_eval<PM, CLS, KIND>(cv, r, zones + i, pf, total);
            // F_BIG records: the integer pass of the caller
            visit(i, ok & want & !((uint32_t)r.flags & F_BIG), total, index_base + (uint32_t)((uint64_t)r.flags >> 32),
                  std::bool_constant<UNI>());
        }
    }
}

// Every record of [lo, hi) a lane wants, once: fast waves on the fast path with their F_BIG records on the integer
// path, the other waves on the integer path (k_select_sets' two loops). Returns the lane's KG_ST_UNSUPPORTED bit over
// its candidate pairs.
template <bool EXACT, bool FAST, uint32_t PM, class F>
__device__ __forceinline__ uint32_t scores_walk(const NodeRec* __restrict__ nodes, const ZoneRec* __restrict__ zones,
                                                const PodV& p, const KCfg& cfg, const uint64_t* __restrict__ srow,
                                                bool live, bool uni, uint32_t lo, uint32_t hi, bool cls1,
                                                uint32_t index_base, F&& visit) {
    bool wave_fast = false;
    if constexpr (FAST) {
        wave_fast = __all(!live || scores_lane_fast(p));
        if (wave_fast) {
            const PodF pf = to_podf(p, cfg);
            const KCfg cv = cfg_in_vgprs(cfg);
            const bool prod = __all(!live || fast_kind_match(FK_PROD, p)), batch = __all(!live || fast_kind_match(FK_BATCH, p));
#define KG_SCORES_LOOP(CLSV, KINDV)                                                                                     \
    do {                                                                                                               \
        if (uni) scores_fast_loop<PM, CLSV, KINDV, true>(nodes, zones, lo, hi, index_base, cv, pf, srow, live, visit);  \
        else scores_fast_loop<PM, CLSV, KINDV, false>(nodes, zones, lo, hi, index_base, cv, pf, srow, live, visit);    \
    } while (0)
            if (!cls1) {
                if (prod) KG_SCORES_LOOP(0, FK_PROD);
                else if (batch) KG_SCORES_LOOP(0, FK_BATCH);
                else KG_SCORES_LOOP(0, FK_ANY);
            } else {
                if (prod) KG_SCORES_LOOP(1, FK_PROD);
                else if (batch) KG_SCORES_LOOP(1, FK_BATCH);
                else KG_SCORES_LOOP(1, FK_ANY);
            }
#undef KG_SCORES_LOOP
        }
    }
    uint32_t unsup = 0;
    for (uint32_t blk = lo >> 6; blk <= (hi - 1u) >> 6; blk++) {
        const uint64_t word = live ? (srow ? srow[blk] : ~0ull) : 0ull;
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
            // per-lane loads: beside eval_pair the load form does not matter
            visit(i, want & (o.status == 0u), (uint32_t)pair_total(cfg, o), rec_gidx(nodes[i], index_base), std::false_type());
        }
    }
    return unsup;
}

// grid (lane blocks, nc0 + nc1): block y < nc0 walks class-0 records [y chunk, ...) of [0, n0), the others class-1
// records of [n0, n_end). PASS 1 writes lmax only; PASS 2 reads it and writes out / pstat (K keys per row).
template <int K, bool EXACT, bool FAST, uint32_t PM, int PASS>
__global__ __launch_bounds__(256) void k_select_scores(const NodeRec* __restrict__ nodes, const ZoneRec* __restrict__ zones,
                                                       PodsDev pods, uint32_t n_lanes, const uint32_t* __restrict__ list,
                                                       const int32_t* __restrict__ pod_set,
                                                       const uint64_t* __restrict__ tab, uint32_t words, ScoresDev sd,
                                                       const int32_t* __restrict__ rtab,  // sd.rtab: see below
                                                       uint32_t* __restrict__ lmax, uint32_t n0, uint32_t n_end,
                                                       uint32_t chunk, uint32_t nc0, uint32_t index_base, KCfg cfg,
                                                       uint64_t* __restrict__ out, uint32_t* __restrict__ pstat) {
    const GridBlock b = xcd_block();  // whole record chunks per XCD (kg_eval.h)
    const uint32_t j = b.x * blockDim.x + threadIdx.x;
    if ((j & ~63u) >= n_lanes) return;  // a wave past the last lane (no barrier below)
    const bool live = j < n_lanes;
    const uint32_t row = live ? list[j] : 0u;
    const WaveTerms w = load_terms(sd, row, live);
    if constexpr (PASS == 1) {
        if (!(w.norm[0] | w.norm[1] | w.norm[2] | w.norm[3])) return;  // wave-uniform: every term of the wave is RAW
    }
    const PodV p = load_pod(pods, row);
    const int32_t set = (live && pod_set) ? pod_set[row] : -1;
    const uint64_t* srow = set >= 0 ? tab + (size_t)set * words : nullptr;
    const bool cls1 = b.y >= nc0;  // uniform
    const uint32_t lo = cls1 ? n0 + (b.y - nc0) * chunk : b.y * chunk;
    const uint32_t hi = cls1 ? min(n_end, lo + chunk) : min(n0, lo + chunk);
    if (lo >= hi) return;
    // rtab is a kernel argument of its own: only a __restrict__ argument is known not to be written by the kernel, and
    // without that a uniform address still gets a vector load (global_load_dword with an SGPR base), no s_load
    const uint32_t n_nodes = sd.n_nodes;
    const bool uni = terms_all_uniform(w);  // decided once per wave
    if constexpr (PASS == 1) {
        uint32_t mx[ST] = {0u, 0u, 0u, 0u};
        scores_walk<EXACT, FAST, PM>(nodes, zones, p, cfg, srow, live, uni, lo, hi, cls1, index_base,
                                     [&](uint32_t i, bool ok, uint32_t, uint32_t, auto u) {
#pragma unroll
                                         for (int t = 0; t < ST; t++) {
                                             if (!w.norm[t]) continue;  // wave-uniform
                                             const uint32_t raw = term_raw<decltype(u)::value>(w, t, rtab, n_nodes, i);
                                             mx[t] = max(mx[t], ok ? raw : 0u);
                                         }
                                     });
#pragma unroll
        for (int t = 0; t < ST; t++)
            if (live && w.mode[t] != KG_SCORE_RAW && mx[t]) atomicMax(lmax + (size_t)j * ST + t, mx[t]);
    } else {
        uint32_t mx[ST];
        float rcp[ST];
#pragma unroll
        for (int t = 0; t < ST; t++) {
            mx[t] = (live && w.mode[t] != KG_SCORE_RAW) ? lmax[(size_t)j * ST + t] : 0u;
            rcp[t] = 1.0f / (float)max(mx[t], 1u);
        }
        uint64_t top[K];
#pragma unroll
        for (int t = 0; t < K; t++) top[t] = 0;
        const uint32_t unsup = scores_walk<EXACT, FAST, PM>(
            nodes, zones, p, cfg, srow, live, uni, lo, hi, cls1, index_base,
            [&](uint32_t i, bool ok, uint32_t total, uint32_t gidx, auto u) {
                // below 2^31 on a feasible candidate (the host checked the bound)
                const uint32_t sum = total + terms_add<decltype(u)::value>(w, mx, rcp, rtab, n_nodes, i);
                const uint64_t key = ((uint64_t)sum << 32) | (uint64_t)(0xFFFFFFFFu - gidx);
                topk_insert<K>(top, ok ? key : 0ull);
            });
        if (live) {
            if constexpr (K == 1) {
                if (top[0]) atomicMax((unsigned long long*)(out + row), (unsigned long long)top[0]);
            } else {
                topk_atomic<K>(out + (size_t)row * K, top);
            }
            if (unsup) atomicOr(pstat + row, unsup);
        }
    }
}

hipError_t launch_select_scores(const NodeRec* nodes, const ZoneRec* zones, const PodsDev& pods, const uint32_t* list,
                                uint32_t n_lanes, const int32_t* pod_set, const uint64_t* tab, uint32_t words,
                                const ScoresDev& sd, uint32_t* lmax, bool norm, uint32_t n0, uint32_t n_nodes,
                                uint32_t index_base, uint32_t k, const KCfg& cfg, bool exact, bool fast, uint64_t* out,
                                uint32_t* pstat, hipStream_t s) {
    if (n_lanes == 0 || n_nodes == 0) return hipSuccess;
    if (!list || !sd.pod_terms || !sd.rtab || !sd.mode || !sd.weight || !lmax || sd.n_nodes != n_nodes || n0 > n_nodes)
        return hipErrorInvalidValue;
    if (pod_set && (!tab || words != (n_nodes + 63u) / 64u)) return hipErrorInvalidValue;
    // about 2048 workgroups; a chunk is at least one table word long (launch_select_sets' geometry)
    const uint32_t lane_blocks = (n_lanes + 255u) / 256u;
    const uint32_t want = max(1u, 2048u / lane_blocks);
    const uint32_t chunk = max(64u, ((n_nodes + want - 1u) / want + 63u) / 64u * 64u);
    const uint32_t nc0 = (n0 + chunk - 1u) / chunk, nc1 = (n_nodes - n0 + chunk - 1u) / chunk;
    if (nc0 + nc1 > 65535u) return hipErrorInvalidValue;
    const dim3 grid(lane_blocks, nc0 + nc1), block(256);
    if (norm) {
        const hipError_t e = hipMemsetAsync(lmax, 0, sizeof(uint32_t) * ST * (size_t)n_lanes, s);
        if (e != hipSuccess) return e;
    }
#define KG_SCORES_ARGS                                                                                                 \
    nodes, zones, pods, n_lanes, list, pod_set, tab, words, sd, sd.rtab, lmax, n0, n_nodes, chunk, nc0, index_base, cfg,   \
        out, pstat
#define KG_SCORES_K(EXACTV, FASTV, PMV)                                                                                \
    do {                                                                                                               \
        if (norm) k_select_scores<1, EXACTV, FASTV, PMV, 1><<<grid, block, 0, s>>>(KG_SCORES_ARGS);                    \
        if (k == 1) k_select_scores<1, EXACTV, FASTV, PMV, 2><<<grid, block, 0, s>>>(KG_SCORES_ARGS);                  \
        else k_select_scores<KG_TOPK_MAX, EXACTV, FASTV, PMV, 2><<<grid, block, 0, s>>>(KG_SCORES_ARGS);               \
    } while (0)
    if (exact) {
        KG_SCORES_K(true, false, 0);
    } else if (!fast) {
        KG_SCORES_K(false, false, 0);
    } else {
        switch (cfg.plugins & 7u) {
            case 0: KG_SCORES_K(false, true, 0); break;
            case 1: KG_SCORES_K(false, true, 1); break;
            case 2: KG_SCORES_K(false, true, 2); break;
            case 3: KG_SCORES_K(false, true, 3); break;
            case 4: KG_SCORES_K(false, true, 4); break;
            case 5: KG_SCORES_K(false, true, 5); break;
            case 6: KG_SCORES_K(false, true, 6); break;
            default: KG_SCORES_K(false, true, 7); break;
        }
    }
#undef KG_SCORES_K
#undef KG_SCORES_ARGS
    return hipGetLastError();
}

// one workgroup per pod row of the verify matrix (snapshot order, like the uploaded raw rows)
__global__ __launch_bounds__(256) void k_scores_verify(ScoresDev sd, uint32_t n_nodes, const uint32_t* __restrict__ status,
                                                       int64_t* __restrict__ total) {
    __shared__ uint32_t s_mx[ST];
    const uint32_t j = blockIdx.x;
    int32_t row[ST];
    uint32_t mode[ST], weight[ST];
    bool any = false;
#pragma unroll
    for (int t = 0; t < ST; t++) {  // uniform over the workgroup
        row[t] = sd.pod_terms[(size_t)j * ST + t];
        mode[t] = row[t] >= 0 ? sd.mode[row[t]] : KG_SCORE_RAW;
        weight[t] = row[t] >= 0 ? sd.weight[row[t]] : 0u;
        any |= row[t] >= 0;
    }
    if (!any) return;
    if (threadIdx.x < ST) s_mx[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t* st = status + (size_t)j * n_nodes;
    uint32_t mx[ST] = {0u, 0u, 0u, 0u};
    for (uint32_t i = threadIdx.x; i < n_nodes; i += 256u) {
        if (st[i] != 0u) continue;
#pragma unroll
        for (int t = 0; t < ST; t++)
            if (row[t] >= 0 && mode[t] != KG_SCORE_RAW) mx[t] = max(mx[t], (uint32_t)sd.raw[(size_t)row[t] * n_nodes + i]);
    }
#pragma unroll
    for (int t = 0; t < ST; t++)
        if (mx[t]) atomicMax(&s_mx[t], mx[t]);
    __syncthreads();
#pragma unroll
    for (int t = 0; t < ST; t++) mx[t] = s_mx[t];
    int64_t* tot = total + (size_t)j * n_nodes;
    for (uint32_t i = threadIdx.x; i < n_nodes; i += 256u) {
        if (st[i] != 0u) continue;
        uint32_t add = 0;
#pragma unroll
        for (int t = 0; t < ST; t++)
            if (row[t] >= 0)
                add += weight[t] * score_term_value(mode[t], (uint32_t)sd.raw[(size_t)row[t] * n_nodes + i], mx[t]);
        tot[i] += (int64_t)add;
    }
}

hipError_t launch_scores_verify(const ScoresDev& sd, uint32_t n_pods, uint32_t n_nodes, const uint32_t* status,
                                int64_t* total, hipStream_t s) {
    if (n_pods == 0 || n_nodes == 0) return hipSuccess;
    if (sd.n_nodes != n_nodes) return hipErrorInvalidValue;
    k_scores_verify<<<dim3(n_pods), 256, 0, s>>>(sd, n_nodes, status, total);
    return hipGetLastError();
}

}  // namespace kg
