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
// A batch with candidate node sets (kg_pods_set_node_sets) adds the pod's set id to the row: two pods share a
// representative only when they also name the same set (-1: none).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace kg {

constexpr int DEDUP_COLS = 9;

struct DedupRows {
    const int64_t* col[DEDUP_COLS];  // each [n]
    const uint32_t* flags;           // [n]
    const int32_t* set;              // [n] candidate node set of the pod, -1 = none; nullptr: the batch carries no sets
};

inline bool dedup_row_equal(const DedupRows& r, uint32_t a, uint32_t b) {
    if (r.flags[a] != r.flags[b]) return false;
    if (r.set && r.set[a] != r.set[b]) return false;
    for (int c = 0; c < DEDUP_COLS; c++)
        if (r.col[c][a] != r.col[c][b]) return false;
    return true;
}

struct DedupHash {
    uint64_t operator()(const DedupRows& r, uint32_t j) const {
        uint64_t h = 0x9E3779B97F4A7C15ull ^ r.flags[j];
        if (r.set) h ^= (uint64_t)(uint32_t)r.set[j] << 32;
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

// Split a lane list (order or rorder: the first n_fast entries fast lanes grouped by wave kind, then the integer lanes)
// of a batch with candidate node sets. Lanes without a set stay in `list`, in their order (plain_fast of them fast):
// the general-path kernels serve them unchanged, over a shorter list. Lanes with a set go to set_list, sorted by (set
// id, fast or integer lane, wave kind) so that a wave's lanes mostly share one set and one loop; kind[row] = the row's
// wave kind (0..2 fast kinds, 3 = integer lane). Returns the number of set lanes.
inline uint32_t dedup_split_sets(uint32_t* list, uint32_t n, uint32_t n_fast, const int32_t* set, const uint8_t* kind,
                                 uint32_t* set_list, uint32_t* plain, uint32_t* plain_fast) {
    uint32_t m = 0, mf = 0, ns = 0;
    for (uint32_t t = 0; t < n; t++) {
        const uint32_t j = list[t];
        if (set[j] >= 0) {
            set_list[ns++] = j;
        } else {
            list[m++] = j;
            if (t < n_fast) mf = m;
        }
    }
    std::stable_sort(set_list, set_list + ns, [&](uint32_t a, uint32_t b) {
        if (set[a] != set[b]) return set[a] < set[b];
        return kind[a] < kind[b];  // the integer kind sorts last: fast lanes, then integer lanes
    });
    *plain = m;
    *plain_fast = mf;
    return ns;
}

// 64-lane waves of a select over n_lanes lanes whose first n_fast are fast lanes (the two groups launch separately)
inline uint32_t dedup_waves(uint32_t n_lanes, uint32_t n_fast) { return (n_fast + 63) / 64 + (n_lanes - n_fast + 63) / 64; }

}  // namespace kg
