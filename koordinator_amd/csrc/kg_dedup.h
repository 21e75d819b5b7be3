// kg_dedup.h — representative rows of a pod batch (host only, no HIP).
//
// The plain select is stateless: every pod is evaluated against the same snapshot and a key holds the total and the
// node index, nothing of the pod. Two pods whose input rows are equal therefore get bit-identical keys and status, so
// the select evaluates one representative per distinct row and k_expand_keys copies its keys to the duplicates.
//
// A row is every per-pod value a plain-path kernel can read. All of them go through load_pod (kg_eval.h) into PodV,
// which eval_pair / to_podf / fast_kind_match consume; no plain-path kernel indexes another per-pod column:
//   the nine int64 columns as staged   req_cpu, req_mem, req_eph, sc_req0, sc_req1, nz_cpu, nz_mem, la_est0, la_est1
//   the flags word as built            KG_POD_* bits (low 16), the pod's NUMA policy (<< 16), POD_FASTV
// (pmap is null on the plain path; the config-5 columns are read by the ext kernels only, and batches that carry them
// are not deduplicated.)
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace kg {

constexpr int DEDUP_COLS = 9;

struct DedupRows {
    const int64_t* col[DEDUP_COLS];  // each [n]
    const uint32_t* flags;           // [n]
};

inline bool dedup_row_equal(const DedupRows& r, uint32_t a, uint32_t b) {
    if (r.flags[a] != r.flags[b]) return false;
    for (int c = 0; c < DEDUP_COLS; c++)
        if (r.col[c][a] != r.col[c][b]) return false;
    return true;
}

struct DedupHash {
    uint64_t operator()(const DedupRows& r, uint32_t j) const {
        uint64_t h = 0x9E3779B97F4A7C15ull ^ r.flags[j];
        for (int c = 0; c < DEDUP_COLS; c++) {
            h ^= (uint64_t)r.col[c][j];
            h *= 0xFF51AFD7ED558CCDull;
            h ^= h >> 32;
        }
        return h;
    }
};

// rep[j] = the lowest row equal to row j (rep[j] == j: a representative). The hash only finds candidates (open
// addressing over representatives); a full row compare decides, so a collision never merges rows. `slots` is scratch
// kept by the caller between calls; nothing of an earlier call survives in it or in rep[0, n). Returns the number of
// representatives.
template <class Hash = DedupHash>
inline uint32_t dedup_rows(const DedupRows& r, uint32_t n, uint32_t* rep, std::vector<uint32_t>& slots, Hash hash = Hash()) {
    size_t cap = 16;
    while (cap < 2 * (size_t)n) cap <<= 1;
    slots.assign(cap, ~0u);
    uint32_t n_rep = 0;
    for (uint32_t j = 0; j < n; j++) {
        size_t at = (size_t)hash(r, j) & (cap - 1);
        for (;;) {
            const uint32_t q = slots[at];
            if (q == ~0u) {  // rows are visited in ascending order: the first of its kind is the lowest
                slots[at] = j;
                rep[j] = j;
                n_rep++;
                break;
            }
            if (dedup_row_equal(r, q, j)) {
                rep[j] = q;
                break;
            }
            at = (at + 1) & (cap - 1);
        }
    }
    return n_rep;
}

// rorder = order restricted to representative rows, grouping kept (equal rows share a wave kind, so a representative
// stands in the group of its duplicates): the fast lanes by wave kind, then the integer lanes in batch order.
inline void dedup_order(const uint32_t* order, uint32_t n, uint32_t n_fast, const uint32_t* rep, uint32_t* rorder,
                        uint32_t* n_rep_fast, uint32_t* n_rep) {
    uint32_t m = 0, mf = 0;
    for (uint32_t t = 0; t < n; t++) {
        const uint32_t j = order[t];
        if (rep[j] != j) continue;
        rorder[m++] = j;
        if (t < n_fast) mf = m;
    }
    *n_rep_fast = mf;
    *n_rep = m;
}

// 64-lane waves of a select over n_lanes lanes whose first n_fast are fast lanes (the two groups launch separately)
inline uint32_t dedup_waves(uint32_t n_lanes, uint32_t n_fast) { return (n_fast + 63) / 64 + (n_lanes - n_fast + 63) / 64; }

}  // namespace kg
