// kg_diag.hip — CDNA4 (gfx950) kernel of the FitError diagnosis (kg_eval_diagnose): per requested pod, how many
// nodes fail with each Filter reason.
//
//   k_diagnose  lane = requested row (a pod of the batch), the wave walks a chunk of node records in uniform order
//               (blockIdx.y = chunk), as k_select's integer path does. Each pair gives two 32-bit words: the counted
//               status word (the pair's KG_ST_* bits, or their first non-empty plugin group) and a derived word
//               (one-hot DeviceShare code, feasible bit). Bit b of a word is counted in byte b / 8 of accumulator
//               b % 8: acc[s] += (w >> s) & 0x01010101, eight adds per word instead of one test-and-add per bit.
//               A byte holds at most 255, so a lane walks at most DIAG_MAX_CHUNK records per launch; the chunk's
//               nonzero counters are then added into the row's KG_DIAG_SLOTS counters by atomicAdd (integer adds:
//               exact in any order).
// The pair's status word comes from row_status (kg_rowfilter.h): kg_eval_verify's bit for bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "kg_diag.h"
#include "kg_rowfilter.h"

namespace kg {

// The framework stops at a node's first failing plugin: the PreFilter gate, then the filter order of
// config/manager/scheduler-config.yaml:69-74. A word with bits of no group (none is defined) stays whole.
__device__ __forceinline__ uint32_t diag_first_plugin(uint32_t w) {
    constexpr uint32_t G[6] = {KG_ST_QUOTA,
                               KG_ST_NRF_MASK,
                               KG_ST_LA_MASK,
                               KG_ST_NUMA_MASK | KG_ST_UNSUPPORTED,
                               KG_ST_DEV_MASK | KG_ST_DEV_RSV,
                               KG_ST_RSV_MASK};
    uint32_t m = w;
#pragma unroll
    for (int g = 5; g >= 0; g--) m = (w & G[g]) ? G[g] : m;
    return w & m;
}

// Derived word of a counted word: bit c = its DeviceShare code is c (1..15), bit 16 = it is 0 (feasible); bit k is
// slot KG_DIAG_DEV_CODE0 + k.
static_assert(KG_DIAG_FEASIBLE - KG_DIAG_DEV_CODE0 == 16 && KG_DIAG_SLOTS == 64, "slot layout of the derived word");
__device__ __forceinline__ uint32_t diag_derived(uint32_t w) {
    const uint32_t code = KG_ST_DEV_CODE(w);
    return (code ? 1u << code : 0u) | (w == 0u ? 1u << 16 : 0u);
}

// Packed counters: byte f of acc[s] counts bit 8 f + s. One add per pair and byte: the launcher keeps a lane's pairs
// per launch at or below DIAG_MAX_CHUNK, so no byte carries into its neighbour.
static_assert(DIAG_MAX_CHUNK <= 255, "a packed 8-bit counter takes one add per record of the chunk");
struct DiagAcc {
    uint32_t w[8], d[8];
};
__device__ __forceinline__ void diag_count(DiagAcc& a, uint32_t w, uint32_t d) {
#pragma unroll
    for (int s = 0; s < 8; s++) {
        a.w[s] += (w >> s) & 0x01010101u;
        a.d[s] += (d >> s) & 0x01010101u;
    }
}

// dst[0..64) += the lane's counters (the nonzero ones: a pod fails with a few reasons)
__device__ __forceinline__ void diag_flush(const DiagAcc& a, uint32_t* __restrict__ dst) {
#pragma unroll
    for (int s = 0; s < 8; s++) {
#pragma unroll
        for (int f = 0; f < 4; f++) {
            const uint32_t cw = (a.w[s] >> (8 * f)) & 0xFFu, cd = (a.d[s] >> (8 * f)) & 0xFFu;
            if (cw) atomicAdd(dst + 8 * f + s, cw);
            if (8 * f + s <= KG_DIAG_FEASIBLE - KG_DIAG_DEV_CODE0 && cd) atomicAdd(dst + KG_DIAG_DEV_CODE0 + 8 * f + s, cd);
        }
    }
}

// Records [begin + chunk * y, ...) of [begin, end) for the rows of block x; counts[t][KG_DIAG_SLOTS] zeroed by the
// launcher. chunk <= DIAG_MAX_CHUNK.
// SETS (plain plugin set only): the batch carries candidate node sets. The lane keeps its set's 64-bit word of the
// record-order table for the 64-record block it walks (reloaded when the wave-uniform record index crosses a block).
// A record outside the set has KG_ST_NODE_EXCLUDED in its word; with first_plugin it is counted under that bit alone
// (the bit belongs to no plugin group, diag_first_plugin would strip it): the host's Filter ran before every koord
// plugin (there is no ElasticQuota gate on the plain path). Without SETS the three arguments are not read.
template <bool EXACT, bool EXT, bool SETS>
__global__ __launch_bounds__(256) void k_diagnose(const NodeRec* __restrict__ nodes, const ZoneRec* __restrict__ zones,
                                                  ExtDev e, PodsDev pods, const uint32_t* __restrict__ rows,
                                                  uint32_t n_rows, uint32_t begin, uint32_t end, uint32_t chunk, KCfg cfg,
                                                  const uint32_t* __restrict__ qst, uint32_t first_plugin,
                                                  uint32_t* __restrict__ counts, const int32_t* __restrict__ pod_set,
                                                  const uint64_t* __restrict__ tab, uint32_t words) {
    const GridBlock b = xcd_block();  // whole record chunks per XCD (kg_eval.h)
    const uint32_t t = b.x * blockDim.x + threadIdx.x;
    if ((t & ~63u) >= n_rows) return;  // uniform: a wave past the last row (no barrier below)
    const bool live = t < n_rows;
    const uint32_t j = live ? (rows ? rows[t] : t) : 0u;
    static_assert(!(EXT && SETS), "candidate node sets are not served on config-5 snapshots");
    const RowCtx c = row_ctx<EXT>(pods, j, live, &e, qst);
    const RowSet rs = row_set<SETS>(pod_set, tab, words, j);
    const uint32_t lo = begin + b.y * chunk;
    const uint32_t hi = min(end, lo + chunk);
    DiagAcc a;
#pragma unroll
    for (int s = 0; s < 8; s++) a.w[s] = a.d[s] = 0u;
    uint64_t cand = ~0ull;
    for (uint32_t rec = lo; rec < hi; rec++) {
        if constexpr (SETS)
            if (rs.set >= 0 && (rec == lo || (rec & 63u) == 0u)) cand = row_cand(rs, rec);
        uint32_t w = row_status<EXACT, EXT, SETS>(cfg, c, nodes[rec].v, zones + rec, rec, cand);
        if (first_plugin) {
            if constexpr (SETS) w = (w & KG_ST_NODE_EXCLUDED) ? (uint32_t)KG_ST_NODE_EXCLUDED : diag_first_plugin(w);
            else w = diag_first_plugin(w);
        }
        diag_count(a, w, diag_derived(w));
    }
    if (live) diag_flush(a, counts + (size_t)t * KG_DIAG_SLOTS);
}

// KG_DIAG_BLOCKS: workgroup target of the launch (tuning aid; 1 gives every lane chunks of DIAG_MAX_CHUNK records).
// Read per call: tests switch it per case.
static uint32_t diag_target_blocks() {
    const char* e = std::getenv("KG_DIAG_BLOCKS");
    const long x = e ? std::strtol(e, nullptr, 10) : 0;
    return (x >= 1 && x <= 65536) ? (uint32_t)x : DIAG_TARGET_BLOCKS;
}

hipError_t launch_diagnose(const RowFilter& f, bool first_plugin, uint32_t* counts, hipStream_t s) {
    if (f.n_rows == 0 || f.n_nodes == 0) return hipSuccess;
    if (!rowfilter_valid(f) || !counts) return hipErrorInvalidValue;
    // whole waves of rows, up to four per workgroup: a short row list leaves no idle wave walking records
    const uint32_t block = std::min<uint32_t>(256u, (f.n_rows + 63u) / 64u * 64u);
    const uint32_t chunk = diag_chunk(f.n_nodes, f.n_rows, block, diag_target_blocks());
    const uint32_t gx = (f.n_rows + block - 1) / block;
    constexpr uint32_t MAX_Y = 65535;  // gridDim.y; larger snapshots take several launches
    for (uint64_t begin = 0; begin < f.n_nodes; begin += (uint64_t)MAX_Y * chunk) {
        const uint32_t end = (uint32_t)std::min<uint64_t>(f.n_nodes, begin + (uint64_t)MAX_Y * chunk);
        const dim3 grid(gx, (end - (uint32_t)begin + chunk - 1) / chunk);
        rowfilter_dispatch(f, [&](auto exact, auto ext, auto sets) {
            k_diagnose<decltype(exact)::value, decltype(ext)::value, decltype(sets)::value><<<grid, block, 0, s>>>(
                f.nodes, f.zones, f.e, f.pods, f.rows, f.n_rows, (uint32_t)begin, end, chunk, f.cfg, f.qst,
                first_plugin ? 1u : 0u, counts, f.pod_set, f.tab, sets_words(f.n_nodes));
        });
        const hipError_t err = hipGetLastError();
        if (err != hipSuccess) return err;
    }
    return hipSuccess;
}

}  // namespace kg
