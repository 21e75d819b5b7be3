// kg_small.h — host arithmetic of the one-pod-block fused top-1 select (k_select_small, kg_kernels.hip):
// the result forms and the status rule, the environment switches, the plan of a launch, and the two pieces of batch
// state that outlive a launch. No HIP include, plain functions over integers: tests/native/small_plan_main.cpp
// compiles them on the host.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "kg_layout.h"  // KG_HD, koordgpu.h; no HIP include either

namespace kg {

constexpr uint32_t SMALL_MAX_CHUNK = 64, SMALL_MAX_CHUNKS = 4096, SMALL_MAX_LANES = 256;
constexpr uint32_t SMALL_WG = 1024;  // most threads of a k_select_small workgroup

// What a launch leaves as its result (LaunchSelect.small_form; DESIGN.md §4, "The forms of the one-launch select"):
//   SLOTS  per-chunk slots, k_small_finish follows as a second launch and writes every row
//   ROWS   one launch, replicated accumulators, the last workgroup to arrive (the finisher) writes every row
//   ROWS4  as ROWS, four rows per thread and step: lane_of, out and pstat are 16-byte aligned
//   LANES  the finisher stores one key and one status word per lane; the reader expands the rows
//   ACC    no finisher: the accumulators are the result, the reader folds the replicas
enum SmallForm : uint32_t { SMALL_SLOTS, SMALL_ROWS, SMALL_ROWS4, SMALL_LANES, SMALL_ACC };

// The status word of a lane from the high word of its best fast key and the highest bound over its pairs found
// KG_ST_UNSUPPORTED (0: none): set when such a pair's bound reaches the best fast key, as k_big_sel would have
// evaluated it. The one rule of k_select_small's finisher, k_small_finish and the host's fold_acc.
KG_HD inline uint32_t small_status(uint32_t fhi, uint32_t ub) { return ub != 0u && ub > fhi ? KG_ST_UNSUPPORTED : 0u; }

inline uint32_t small_lp(uint32_t n_fast) { return (n_fast + 63u) / 64u * 64u; }  // lanes rounded up to whole waves

// The environment switches of this path. RULE: all nine are read per call, by small_switches() and nowhere else, so a
// test or a tool may set and unset them between two selects of one process; everything downstream takes the struct.
struct SmallSwitches {
    bool off = false;              // KG_NO_SMALL_SELECT: the general path
    bool allow_big = false;        // KG_SMALL_ALLOW_BIG: lifts the F_BIG gate (the A/B tool and the tests)
    bool no_fused_finish = false;  // KG_NO_SMALL_FUSED_FINISH: SLOTS always
    bool finisher = false;         // KG_SMALL_FINISHER: LANES where ACC would run
    bool row_results = false;      // KG_SMALL_ROW_RESULTS: the caller keeps rows where it could keep lanes
    bool bound_events = false;     // KG_PROFILE_BOUND_EVENTS: the bound event pair where the device clock would time
    uint32_t replicas = 0;         // KG_SMALL_REPLICAS=<n >= 1>: the replica count, also past the row gate (0: unset)
    bool has_chunks = false;       // KG_SMALL_CHUNKS="c0,c1,copies" parsed into chunks[] (measurement aid)
    uint32_t chunks[3] = {0, 0, 0};
    const char* phases = nullptr;  // KG_SMALL_PHASES=<file>: the PH instantiation's readings go there (measurement aid)
};
inline SmallSwitches small_switches() {
    SmallSwitches sw;
    sw.off = std::getenv("KG_NO_SMALL_SELECT") != nullptr;
    sw.allow_big = std::getenv("KG_SMALL_ALLOW_BIG") != nullptr;
    sw.no_fused_finish = std::getenv("KG_NO_SMALL_FUSED_FINISH") != nullptr;
    sw.finisher = std::getenv("KG_SMALL_FINISHER") != nullptr;
    sw.row_results = std::getenv("KG_SMALL_ROW_RESULTS") != nullptr;
    sw.bound_events = std::getenv("KG_PROFILE_BOUND_EVENTS") != nullptr;
    unsigned v = 0, c[3] = {0, 0, 0};
    if (const char* e = std::getenv("KG_SMALL_REPLICAS"))
        if (std::sscanf(e, "%u", &v) == 1 && v >= 1) sw.replicas = v;
    if (const char* e = std::getenv("KG_SMALL_CHUNKS")) sw.has_chunks = std::sscanf(e, "%u,%u,%u", &c[0], &c[1], &c[2]) == 3;
    for (int i = 0; i < 3; i++) sw.chunks[i] = c[i];
    const char* f = std::getenv("KG_SMALL_PHASES");
    sw.phases = f && *f ? f : nullptr;
    return sw;
}

// What the plan is a function of: the launch's counts, the snapshot's F_BIG estimate and the device.
struct SmallShape {
    uint32_t k = 0;
    bool fused = false;
    uint32_t n_pods = 0, n_fast = 0, n_rows = 0;  // lanes, fast lanes, rows
    uint32_t len[2] = {0, 0};                     // records of storage class 0 / 1
    uint32_t n_big_est = 0, n_nodes = 0, cus = 0;  // cus: compute units the device reports (0: unknown)
    bool lanes_ok = false, aligned16 = false;  // the caller can keep lanes; lane_of, out and pstat are 16-byte aligned
};
struct SmallPlan {
    bool take = false;  // else the general path, and nothing below counts
    uint32_t chunk[2] = {0, 0}, n_chunks[2] = {0, 0}, slices = 0;  // slices: copies of the lanes per workgroup
    SmallForm form = SMALL_SLOTS;
    uint32_t replicas = 0;  // 0 exactly for SMALL_SLOTS
};

// threads that the copies of the lanes may fill (512: the launch-bound variant without scratch; 1024: the spilling one)
constexpr uint32_t SMALL_COPIES_WG = 1024, SMALL_BIG_DEN = 250, SMALL_BIG_EVEN_DEN = 400;
constexpr uint32_t SMALL_MIN_CHUNK = 8, SMALL_FILL_NUM = 63, SMALL_FILL_DEN = 64, SMALL_MIN_CUS = 8;
constexpr uint32_t SMALL_REPLICAS = 4, SMALL_ACC_REPLICAS = 4, SMALL_FUSED_MAX_ROWS = 32768;
constexpr uint32_t SMALL_ACC_SLOTS = 2048;  // replicas x lanes (whole waves) of one ACC launch at most

// The gates that need no switch: top-1, fused, every lane a fast lane and at most 256 of them.
inline bool small_shape_ok(const SmallShape& in) {
    return in.k == 1 && in.fused && in.n_fast != 0 && in.n_fast == in.n_pods && in.n_fast <= SMALL_MAX_LANES;
}

// The plan of one select; the measurements behind every rule are in DESIGN.md §4. F_BIG gate: at most 1 F_BIG record in
// SMALL_BIG_DEN unless allow_big. Geometry: one round of workgroups. Wide rule: a class-1 chunk half a class-0 one, 63/64
// of the compute units, a count in (CUs, 2 CUs) lengthened out of it (unreachable with this fill: the rounded counts
// stay within one of the count asked for; kept for a change of fill, and the host test notices if it comes alive).
// Narrow rule (one wave of lanes, or F_BIG records above 1 in SMALL_BIG_EVEN_DEN): 3/4 as long, 7/8 of the units.
// Form: ACC where the caller keeps lanes (LANES with the finisher switch), else rows up to SMALL_FUSED_MAX_ROWS, SLOTS
// beyond; a replica override applies past the row gate too.
inline SmallPlan small_plan(const SmallShape& in, const SmallSwitches& sw) {
    SmallPlan pl;
    if (!small_shape_ok(in) || sw.off) return pl;
    if ((uint64_t)in.n_big_est * SMALL_BIG_DEN > in.n_nodes && !sw.allow_big) return pl;
    const uint32_t lp = small_lp(in.n_fast), len0 = in.len[0], len1 = in.len[1];
    const uint32_t cus = std::max(in.cus, SMALL_MIN_CUS);
    const bool narrow = lp <= 64 || (uint64_t)in.n_big_est * SMALL_BIG_EVEN_DEN > in.n_nodes;
    const uint32_t want = std::max<uint32_t>(1u, narrow ? cus * 7 / 8 : cus * SMALL_FILL_NUM / SMALL_FILL_DEN);
    // a class-1 chunk is rn / rd as long as a class-0 one; the work in 1 / rn of a class-0 record
    const uint32_t rn = narrow ? 3 : 1, rd = narrow ? 4 : 2;
    const uint64_t work = (uint64_t)len0 * rn + (uint64_t)len1 * rd;
    const auto chunk1_of = [&](uint32_t c0) { return std::max<uint32_t>(1u, narrow ? c0 * 3 / 4 : (c0 + 1) / 2); };
    const auto chunks_at = [&](uint32_t c0) { return (len0 + c0 - 1) / c0 + (len1 + chunk1_of(c0) - 1) / chunk1_of(c0); };
    uint32_t c0 = (uint32_t)std::min<uint64_t>(
        SMALL_MAX_CHUNK, std::max<uint64_t>(SMALL_MIN_CHUNK, (work + (uint64_t)rn * want - 1) / ((uint64_t)rn * want)));
    while (!narrow && c0 < SMALL_MAX_CHUNK && chunks_at(c0) > cus && chunks_at(c0) < 2 * cus) c0++;
    uint32_t c1 = chunk1_of(c0);
    pl.slices = SMALL_COPIES_WG / lp;
    const uint32_t* e = sw.chunks;
    if (sw.has_chunks && e[0] >= 1 && e[0] <= SMALL_MAX_CHUNK && e[1] >= 1 && e[1] <= SMALL_MAX_CHUNK && e[2] >= 1 &&
        (uint64_t)e[2] * lp <= SMALL_WG) {
        c0 = e[0];
        c1 = e[1];
        pl.slices = e[2];
    }
    pl.chunk[0] = c0;
    pl.chunk[1] = c1;
    pl.n_chunks[0] = (len0 + c0 - 1) / c0;
    pl.n_chunks[1] = (len1 + c1 - 1) / c1;
    const uint32_t nc = pl.n_chunks[0] + pl.n_chunks[1];
    pl.take = nc != 0 && nc <= SMALL_MAX_CHUNKS;
    if (!pl.take || sw.no_fused_finish) return pl;
    const bool acc = in.lanes_ok && !sw.finisher;
    uint32_t rep = acc ? SMALL_ACC_REPLICAS : in.lanes_ok || in.n_rows <= SMALL_FUSED_MAX_ROWS ? SMALL_REPLICAS : 0u;
    if (sw.replicas) rep = sw.replicas;
    pl.replicas = std::min(rep, nc);  // more replicas than chunks: one chunk each
    if (acc) pl.replicas = std::min(pl.replicas, SMALL_ACC_SLOTS / lp);
    if (pl.replicas) pl.form = acc ? SMALL_ACC : in.lanes_ok ? SMALL_LANES : in.aligned16 ? SMALL_ROWS4 : SMALL_ROWS;
    return pl;
}

// The result accumulators of the ACC form: two parities of SMALL_ACC_SLOTS 16-byte words in one buffer.
// INVARIANT: when no select runs on the batch and !clear, parity `par` is all zero and the other one is zero past its
// first dirty[par ^ 1] words. A launch accumulates into `par` and zeroes the other parity's dirty words at its entry
// (same-stream order: the launch that dirtied them, and the copy that read them, are through); launched() then swaps
// the parities. The arrays of a launch start at the parity's base whatever its replica and lane counts, so the dirty
// words are a prefix. clear: the whole buffer needs the memset, then cleared(): at allocation and after failed().
struct AccParity {
    bool clear = true;
    uint32_t par = 0, dirty[2] = {0, 0};
    struct Next {
        size_t mine, other;  // byte offsets of the parity to accumulate into and of the one to zero
        uint32_t zero_n;     // 16-byte words to zero at `other`
    };
    static size_t base(uint32_t parity) { return (size_t)parity * SMALL_ACC_SLOTS * 16; }
    Next next() const { return {base(par), base(par ^ 1u), dirty[par ^ 1u]}; }  // what the next launch gets (!clear)
    void cleared() { clear = false, dirty[0] = dirty[1] = 0; }
    void launched(uint32_t slots) { dirty[par] = slots, dirty[par ^ 1u] = 0, par ^= 1u; }  // replicas x lp words dirty
    void failed() { clear = true; }  // a failed call may have left a launch half done
};

// The staged accumulators of an ACC select, [r][lp] keys, [r][lp] fast-key high words, [r][lp] unsupported bounds,
// become the lane tables in place: per lane the maximum over the replicas and the status rule. The keys of replica 0
// are the key table; the status words take the place of replica 0's high words. Returns their place in 64-bit words.
inline uint32_t fold_acc(uint64_t* keys, uint32_t r, uint32_t lp) {
    uint32_t* fhi = reinterpret_cast<uint32_t*>(keys + (size_t)r * lp);
    const uint32_t* ub = fhi + (size_t)r * lp;
    for (uint32_t j = 0; j < lp; j++) {
        uint64_t k = keys[j];
        uint32_t f = fhi[j], u = ub[j];
        for (uint32_t q = 1; q < r; q++) {
            const size_t at = (size_t)q * lp + j;
            k = std::max(k, keys[at]);
            f = std::max(f, fhi[at]);
            u = std::max(u, ub[at]);
        }
        keys[j] = k;
        fhi[j] = small_status(f, u);
    }
    return r * lp;
}

// A result kept per lane (LANES, ACC): row j takes lane lane_of[j], the host's copy of the row -> lane table of the
// select's upload. LANES: dev holds lp keys and, behind them, lp status words. ACC (acc_r > 0): acc_r x lp x 16 bytes at
// acc, the launch's parity. The readers copy either into host once per select (fetched) and fold() makes the lane
// tables; stat_at: the status words' place in host, in 64-bit words. dev / host: staging of SMALL_LRES_WORDS words.
constexpr uint32_t SMALL_LRES_WORDS = 2 * SMALL_ACC_SLOTS;  // 64-bit words
static_assert(SMALL_LRES_WORDS >= SMALL_MAX_LANES + SMALL_MAX_LANES / 2 && SMALL_ACC_SLOTS >= SMALL_MAX_LANES,
              "the staging holds either form");
struct LaneResult {
    uint64_t *dev = nullptr, *host = nullptr;
    bool lanes = false, fetched = false;
    uint32_t lp = 0, acc_r = 0, stat_at = 0;
    const uint8_t *acc = nullptr, *lane_of = nullptr;
    void reset() { lanes = fetched = false, acc_r = 0; }
    // the launch is on the stream (replicas = 0: LANES)
    void claim(uint32_t lanes_padded, const uint8_t* host_lane_of, uint32_t replicas, const void* accumulators) {
        *this = {dev, host, true, false, lanes_padded, replicas, lanes_padded, static_cast<const uint8_t*>(accumulators), host_lane_of};
    }
    size_t fetch_bytes() const { return acc_r ? (size_t)16 * acc_r * lp : (sizeof(uint64_t) + sizeof(uint32_t)) * lp; }
    void fold() {  // once per select, after the copy
        if (!fetched && acc_r) stat_at = fold_acc(host, acc_r, lp);
        fetched = true;
    }
    const uint32_t* status() const { return reinterpret_cast<const uint32_t*>(host + stat_at); }
};

}  // namespace kg
