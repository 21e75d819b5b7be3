// kg_feasible.hip — CDNA4 (gfx950) kernels of the feasible-node bitmaps (kg_eval_feasible): per requested pod, one bit
// per node of the snapshot: the pair's status word has no bit of the caller's fail_mask.
//
// Records are stored in storage-class order, the output is in snapshot order: two steps, no per-pair atomics.
//   step 1  the record-order bitmap rtab[row][ceil(n / 64)], bit (r & 63) of word (r >> 6) = the pair at record
//           position r. Two forms:
//     k_feasible_by_rows     lane = requested row, the wave walks a chunk of records in uniform order (blockIdx.y =
//                            chunk; the record index is wave-uniform, record loads stay scalar), k_diagnose's geometry.
//                            Chunks start at multiples of 64 records, so a lane ORs 64 pairs into a register and stores
//                            the word: one writer per word, plain stores.
//     k_feasible_by_records  lane = record, the pod row is wave-uniform (blockIdx.y = row): the ballot of a wave's 64
//                            consecutive records is the word, one lane stores it. For the few-row calls (the
//                            framework's cycle asks for one pod), where lane = row leaves most lanes idle.
//   step 2  k_feasible_rows  the inverse of k_sets_table: lane = snapshot position i of one row reads the bit of record
//                            position pos[i]; the ballot's halves are two 32-bit output words.
// The pair's status word comes from row_status (kg_rowfilter.h), as k_diagnose's with flags 0: kg_eval_verify's bit for
// bit. No MFMA: integer / IEEE-double scalar work.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "kg_feasible.h"
#include "kg_rowfilter.h"

namespace kg {

// Records [begin + chunk * y, ...) of [begin, end) for the rows of block x. begin and chunk are multiples of 64.
// SETS (plain plugin set only): the lane keeps its set's word of the record-order table for the 64 records it walks.
// Without SETS pod_set and tab are not read; without EXT e and qst are not.
template <bool EXACT, bool EXT, bool SETS>
__global__ __launch_bounds__(256) void k_feasible_by_rows(const NodeRec* __restrict__ nodes,
                                                          const ZoneRec* __restrict__ zones, ExtDev e, PodsDev pods,
                                                          const uint32_t* __restrict__ rows, uint32_t n_rows,
                                                          uint32_t begin, uint32_t end, uint32_t chunk, KCfg cfg,
                                                          const uint32_t* __restrict__ qst, uint32_t fail_mask,
                                                          uint64_t* __restrict__ rtab, const int32_t* __restrict__ pod_set,
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
    uint64_t* __restrict__ dst = rtab + (size_t)(live ? t : 0u) * words;
    for (uint32_t w0 = lo; w0 < hi; w0 += 64u) {  // one word of the row: records [w0, w1), w0 a multiple of 64
        const uint32_t w1 = min(hi, w0 + 64u);
        const uint64_t cand = row_cand(rs, w0);
        uint64_t acc = 0ull;
        for (uint32_t rec = w0; rec < w1; rec++) {
            const uint32_t st = row_status<EXACT, EXT, SETS>(cfg, c, nodes[rec].v, zones + rec, rec, cand);
            acc |= (uint64_t)((st & fail_mask) == 0u) << (rec & 63u);
        }
        if (live) dst[w0 >> 6] = acc;
    }
}

// grid (ceil(n_nodes / 256), rows of this launch): wave w of block x builds word 4 x + w of row row_base + y.
template <bool EXACT, bool EXT, bool SETS>
__global__ __launch_bounds__(256) void k_feasible_by_records(const NodeRec* __restrict__ nodes,
                                                             const ZoneRec* __restrict__ zones, ExtDev e, PodsDev pods,
                                                             const uint32_t* __restrict__ rows, uint32_t row_base,
                                                             uint32_t n_nodes, KCfg cfg, const uint32_t* __restrict__ qst,
                                                             uint32_t fail_mask, uint64_t* __restrict__ rtab,
                                                             const int32_t* __restrict__ pod_set,
                                                             const uint64_t* __restrict__ tab, uint32_t words) {
    const uint32_t rec = blockIdx.x * 256u + threadIdx.x;
    const uint32_t t = row_base + blockIdx.y;
    const uint32_t j = rows ? rows[t] : t;  // uniform over the workgroup
    bool ok = false;
    if (rec < n_nodes) {
        static_assert(!(EXT && SETS), "candidate node sets are not served on config-5 snapshots");
        const RowCtx c = row_ctx<EXT>(pods, j, true, &e, qst);
        uint32_t st = row_status<EXACT, EXT, false>(cfg, c, nodes[rec].v, zones + rec, rec, ~0ull);
        // the set and its candidate word (uniform over the wave) are fetched after the evaluation
        if constexpr (SETS) st = row_exclude(st, row_set<true>(pod_set, tab, words, j), rec);
        ok = (st & fail_mask) == 0u;
    }
    const uint64_t word = __ballot(ok);
    const uint32_t w = rec >> 6;  // uniform over the wave
    if ((threadIdx.x & 63u) == 0u && w < words) rtab[(size_t)t * words + w] = word;
}

// grid (ceil(n_nodes / 256), ceil(rows of this launch / FEAS_ROWS_PER_BLOCK)): lane = snapshot position i; the
// workgroup loads its positions' record positions once and serves rows [row_base + y R, ... + R) with them.
__global__ __launch_bounds__(256) void k_feasible_rows(const uint64_t* __restrict__ rtab, const uint32_t* __restrict__ pos,
                                                       uint32_t row_base, uint32_t n_rows, uint32_t n_nodes,
                                                       uint32_t words, uint32_t words32, uint32_t* __restrict__ out,
                                                       uint32_t* __restrict__ count) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const bool live = i < n_nodes;
    const uint32_t r = live ? pos[i] : 0u;  // < n_nodes
    const uint32_t w = i >> 5;              // the wave's first output word (even; uniform over the wave)
    const uint32_t t0 = row_base + blockIdx.y * FEAS_ROWS_PER_BLOCK;
    const uint32_t t1 = min(n_rows, t0 + FEAS_ROWS_PER_BLOCK);
    for (uint32_t t = t0; t < t1; t++) {
        const bool bit = live && ((rtab[(size_t)t * words + (r >> 6)] >> (r & 63u)) & 1ull);
        const uint64_t m = __ballot(bit);  // lanes at or above n_nodes: 0, the padding of the last word
        if ((threadIdx.x & 63u) == 0u && w < words32) {
            uint32_t* __restrict__ dst = out + (size_t)t * words32;
            dst[w] = (uint32_t)m;
            if (w + 1u < words32) dst[w + 1u] = (uint32_t)(m >> 32);
            if (count && m) atomicAdd(count + t, (uint32_t)__popcll(m));
        }
    }
}

// KG_FEASIBLE_FORM=rows|records: force a form of step 1 (the rate tool and the tests). Read per call.
static bool feasible_by_rows(uint32_t n_rows, uint32_t n_nodes) {
    const char* e = std::getenv("KG_FEASIBLE_FORM");
    if (e && std::strcmp(e, "rows") == 0) return true;
    if (e && std::strcmp(e, "records") == 0) return false;
    return feasible_rows_form(n_rows, n_nodes);
}

hipError_t launch_feasible_records(const RowFilter& f, uint32_t fail_mask, uint64_t* rtab, hipStream_t s) {
    const uint32_t n_rows = f.n_rows, n_nodes = f.n_nodes;
    if (n_rows == 0 || n_nodes == 0) return hipSuccess;
    if (!rowfilter_valid(f) || !rtab) return hipErrorInvalidValue;
    const uint32_t words = feasible_words(n_nodes);  // rtab's row and, as sets_words(n_nodes), the table's
    if (feasible_by_rows(n_rows, n_nodes)) {
        // whole waves of rows, up to four per workgroup: a short row list leaves no idle wave walking records
        const uint32_t block = std::min<uint32_t>(256u, (n_rows + 63u) / 64u * 64u);
        const uint32_t chunk = feasible_chunk(n_nodes, n_rows, block);
        const uint32_t gx = (n_rows + block - 1) / block;
        for (uint64_t begin = 0; begin < n_nodes; begin += feasible_span(chunk)) {
            const uint32_t end = (uint32_t)std::min<uint64_t>(n_nodes, begin + feasible_span(chunk));
            const dim3 grid(gx, (end - (uint32_t)begin + chunk - 1) / chunk);
            rowfilter_dispatch(f, [&](auto exact, auto ext, auto sets) {
                k_feasible_by_rows<decltype(exact)::value, decltype(ext)::value, decltype(sets)::value>
                    <<<grid, block, 0, s>>>(f.nodes, f.zones, f.e, f.pods, f.rows, n_rows, (uint32_t)begin, end, chunk,
                                            f.cfg, f.qst, fail_mask, rtab, f.pod_set, f.tab, words);
            });
            const hipError_t err = hipGetLastError();
            if (err != hipSuccess) return err;
        }
        return hipSuccess;
    }
    const uint32_t gx = (n_nodes + 255u) / 256u;
    for (uint32_t base = 0; base < n_rows; base += std::min(n_rows - base, FEAS_MAX_Y)) {
        const dim3 grid(gx, std::min(n_rows - base, FEAS_MAX_Y));
        rowfilter_dispatch(f, [&](auto exact, auto ext, auto sets) {
            k_feasible_by_records<decltype(exact)::value, decltype(ext)::value, decltype(sets)::value>
                <<<grid, 256, 0, s>>>(f.nodes, f.zones, f.e, f.pods, f.rows, base, n_nodes, f.cfg, f.qst, fail_mask, rtab,
                                      f.pod_set, f.tab, words);
        });
        const hipError_t err = hipGetLastError();
        if (err != hipSuccess) return err;
    }
    return hipSuccess;
}

hipError_t launch_feasible_rows(const uint64_t* rtab, const uint32_t* pos, uint32_t n_rows, uint32_t n_nodes,
                                uint32_t* out, uint32_t* count, hipStream_t s) {
    if (n_rows == 0 || n_nodes == 0) return hipSuccess;
    if (!rtab || !pos || !out) return hipErrorInvalidValue;
    const uint32_t gx = (n_nodes + 255u) / 256u;
    constexpr uint32_t SPAN = FEAS_MAX_Y * FEAS_ROWS_PER_BLOCK;  // rows of one launch
    for (uint32_t base = 0; base < n_rows; base += std::min(n_rows - base, SPAN)) {
        const uint32_t r = std::min(n_rows - base, SPAN);
        k_feasible_rows<<<dim3(gx, (r + FEAS_ROWS_PER_BLOCK - 1u) / FEAS_ROWS_PER_BLOCK), 256, 0, s>>>(
            rtab, pos, base, n_rows, n_nodes, feasible_words(n_nodes), feasible_words32(n_nodes), out, count);
        const hipError_t err = hipGetLastError();
        if (err != hipSuccess) return err;
    }
    return hipSuccess;
}

}  // namespace kg
