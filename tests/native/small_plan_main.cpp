// Stand-alone host test of koordinator_amd/csrc/kg_small.h: the plan of the one-pod-block select (pinned from
// DESIGN.md §4), the switches, the accumulator parity model over a host array, and fold_acc against a brute force.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../koordinator_amd/csrc/kg_small.h"

using namespace kg;

static int failures = 0;
#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
            failures++;                                               \
        }                                                             \
    } while (0)

// config 2's launch: 8,000 class-0 and 2,000 class-1 records, 10,000 rows, 256 compute units
static SmallShape shape(uint32_t lanes, bool lanes_ok = true) {
    SmallShape in;
    in.k = 1;
    in.fused = true;
    in.n_pods = in.n_fast = lanes;
    in.n_rows = 10000;
    in.len[0] = 8000;
    in.len[1] = 2000;
    in.n_nodes = 10000;
    in.cus = 256;
    in.lanes_ok = lanes_ok;
    in.aligned16 = true;
    return in;
}

static void test_geometry() {
    const SmallSwitches sw;
    SmallPlan pl = small_plan(shape(145), sw);
    CHECK(pl.take && pl.chunk[0] == 48 && pl.chunk[1] == 24 && pl.n_chunks[0] == 167 && pl.n_chunks[1] == 84);
    CHECK(pl.slices == 5 && pl.form == SMALL_ACC && pl.replicas == 4);
    pl = small_plan(shape(64), sw);
    CHECK(pl.take && pl.chunk[0] == 48 && pl.chunk[1] == 36 && pl.n_chunks[0] + pl.n_chunks[1] == 223 && pl.slices == 16);
    // F_BIG estimate x 400 > nodes selects the narrow rule; x 250 > nodes closes the path unless allowed
    SmallShape big = shape(145);
    big.n_big_est = 26;
    pl = small_plan(big, sw);
    CHECK(pl.take && pl.chunk[0] == 48 && pl.chunk[1] == 36);
    big.n_big_est = 25;
    pl = small_plan(big, sw);
    CHECK(pl.take && pl.chunk[1] == 24);
    big.n_big_est = 41;
    CHECK(!small_plan(big, sw).take);
    SmallSwitches allow;
    allow.allow_big = true;
    pl = small_plan(big, allow);
    CHECK(pl.take && pl.chunk[1] == 36);
    big.n_big_est = 40;
    CHECK(small_plan(big, sw).take);
    // fewer than 8 compute units reported counts as 8
    SmallShape few = shape(145);
    few.len[0] = 300;
    few.len[1] = 60;
    few.cus = 8;
    const SmallPlan p8 = small_plan(few, sw);
    for (uint32_t cus = 0; cus < 8; cus++) {
        few.cus = cus;
        pl = small_plan(few, sw);
        CHECK(pl.take && pl.chunk[0] == p8.chunk[0] && pl.chunk[1] == p8.chunk[1] && pl.n_chunks[0] == p8.n_chunks[0]);
    }
    // more than 4,096 chunks: no small path
    SmallShape huge = shape(145);
    huge.len[0] = 64 * 4096;
    huge.len[1] = 0;
    CHECK(small_plan(huge, sw).take);
    huge.len[0]++;
    CHECK(!small_plan(huge, sw).take);
    huge.len[0] = huge.len[1] = 0;
    CHECK(!small_plan(huge, sw).take);
    // a sweep of class lengths and devices: lengths in [8, 64]; a count in (CUs, 2 CUs) is lengthened out of it on the
    // wide rule only (the chunk the fill asks for is recomputed here)
    uint32_t lengthened = 0, narrow_inside = 0;
    for (uint32_t lanes : {64u, 145u})
        for (uint32_t cus : {8u, 64u, 256u, 304u})
            for (uint32_t len0 = 0; len0 <= 40000; len0 += len0 < 1500 ? 7 : 371)
                for (uint32_t len1 = 0; len1 <= 12000; len1 += len1 < 800 ? 13 : 997) {
                    if (len0 + len1 == 0) continue;
                    SmallShape in = shape(lanes);
                    in.len[0] = len0;
                    in.len[1] = len1;
                    in.cus = cus;
                    pl = small_plan(in, sw);
                    const bool narrow = lanes <= 64;
                    const uint64_t want = narrow ? cus * 7 / 8 : cus * 63 / 64, rn = narrow ? 3 : 1, rd = narrow ? 4 : 2;
                    const uint64_t asked = std::min<uint64_t>(
                        64, std::max<uint64_t>(8, ((uint64_t)len0 * rn + (uint64_t)len1 * rd + rn * want - 1) / (rn * want)));
                    const uint32_t nc = pl.n_chunks[0] + pl.n_chunks[1];
                    if (!pl.take) {
                        CHECK((len0 + 63) / 64 + (len1 + 31) / 32 > 4096 || nc > 4096);
                        continue;
                    }
                    CHECK(pl.chunk[0] >= 8 && pl.chunk[0] <= 64 && pl.chunk[1] >= 1 && pl.chunk[1] <= 64);
                    CHECK(pl.chunk[1] == (narrow ? pl.chunk[0] * 3 / 4 : (pl.chunk[0] + 1) / 2));
                    CHECK(pl.n_chunks[0] == (len0 + pl.chunk[0] - 1) / pl.chunk[0]);
                    CHECK(pl.n_chunks[1] == (len1 + pl.chunk[1] - 1) / pl.chunk[1]);
                    const bool inside = nc > cus && nc < 2 * cus;
                    if (narrow) {
                        CHECK(pl.chunk[0] == asked);
                        narrow_inside += inside;
                    } else {
                        CHECK(pl.chunk[0] >= asked && (!inside || pl.chunk[0] == 64));
                        lengthened += pl.chunk[0] > asked;
                    }
                }
    // Wide rule, 63/64 fill: the two rounded counts stay within one of the count asked for, which is below the compute
    // units, so no input reaches the interval and the lengthening is unreachable; a change of fill that revives it
    // fails here. Narrow rule: its 3/4 is rounded down, plans do land in the interval, and none of them is lengthened
    // (chunk == asked above): on the wide rule only.
    CHECK(lengthened == 0 && narrow_inside > 0);
}

static void test_gates_and_forms() {
    const SmallSwitches sw;
    SmallShape in = shape(145);
    in.k = 2;
    CHECK(!small_plan(in, sw).take);
    in = shape(145);
    in.fused = false;
    CHECK(!small_plan(in, sw).take);
    in = shape(145);
    in.n_pods = 146;  // an integer lane present
    CHECK(!small_plan(in, sw).take);
    CHECK(!small_plan(shape(257), sw).take && small_plan(shape(256), sw).take && !small_plan(shape(0), sw).take);
    SmallSwitches off;
    off.off = true;
    CHECK(!small_plan(shape(145), off).take);
    // lanes_ok: ACC, R = min(4, chunks, 2048 / lp)
    SmallPlan pl = small_plan(shape(256), sw);
    CHECK(pl.form == SMALL_ACC && pl.replicas == 4);
    in = shape(145);
    in.len[0] = 20;
    in.len[1] = 0;
    pl = small_plan(in, sw);
    CHECK(pl.take && pl.form == SMALL_ACC && pl.n_chunks[0] + pl.n_chunks[1] == 3 && pl.replicas == 3);
    SmallSwitches rep;
    rep.replicas = 4000;  // the override is capped the same way: 2048 / 192 = 10, 2048 / 256 = 8, one per chunk
    CHECK(small_plan(shape(145), rep).replicas == 10 && small_plan(shape(256), rep).replicas == 8);
    CHECK(small_plan(in, rep).replicas == 3);
    // with the finisher switch: LANES, R = min(4, chunks), the override up to one per chunk
    SmallSwitches fin;
    fin.finisher = true;
    pl = small_plan(shape(145), fin);
    CHECK(pl.form == SMALL_LANES && pl.replicas == 4 && small_plan(in, fin).replicas == 3);
    fin.replicas = 4000;
    CHECK(small_plan(shape(145), fin).replicas == 251);
    // not lanes_ok: rows from the finisher up to 32,768 rows, four at a time if aligned; beyond: slots
    in = shape(145, false);
    pl = small_plan(in, sw);
    CHECK(pl.form == SMALL_ROWS4 && pl.replicas == 4);
    in.aligned16 = false;
    CHECK(small_plan(in, sw).form == SMALL_ROWS);
    in.n_rows = 32768;
    CHECK(small_plan(in, sw).form == SMALL_ROWS);
    in.n_rows = 32769;
    pl = small_plan(in, sw);
    CHECK(pl.take && pl.form == SMALL_SLOTS && pl.replicas == 0);
    rep.replicas = 7;  // a replica override applies past the row gate too
    pl = small_plan(in, rep);
    CHECK(pl.form == SMALL_ROWS && pl.replicas == 7);
    in.n_rows = 200000;
    in.lanes_ok = true;  // the lane forms store no row: no row gate
    CHECK(small_plan(in, sw).form == SMALL_ACC && small_plan(in, fin).form == SMALL_LANES);
    // the no-fused-finish switch: SLOTS always
    SmallSwitches two;
    two.no_fused_finish = true;
    two.replicas = 5;
    for (bool ok : {false, true}) {
        pl = small_plan(shape(145, ok), two);
        CHECK(pl.take && pl.form == SMALL_SLOTS && pl.replicas == 0);
    }
    // KG_SMALL_CHUNKS: all three fields in range and copies x lp <= 1,024, else the plan's own geometry
    const auto with_chunks = [&](uint32_t c0, uint32_t c1, uint32_t copies, uint32_t lanes) {
        SmallSwitches c;
        c.has_chunks = true;
        c.chunks[0] = c0;
        c.chunks[1] = c1;
        c.chunks[2] = copies;
        return small_plan(shape(lanes), c);
    };
    pl = with_chunks(7, 5, 2, 145);
    CHECK(pl.chunk[0] == 7 && pl.chunk[1] == 5 && pl.slices == 2 && pl.n_chunks[0] == 1143 && pl.n_chunks[1] == 400);
    pl = with_chunks(64, 64, 5, 145);
    CHECK(pl.chunk[0] == 64 && pl.slices == 5);
    for (const SmallPlan& q : {with_chunks(0, 5, 2, 145), with_chunks(65, 5, 2, 145), with_chunks(7, 0, 2, 145),
                               with_chunks(7, 65, 2, 145), with_chunks(7, 5, 0, 145), with_chunks(7, 5, 6, 145),
                               with_chunks(7, 5, 0x40000000u, 145)})
        CHECK(q.take && q.chunk[0] == 48 && q.chunk[1] == 24 && q.slices == 5);
    CHECK(with_chunks(8, 8, 16, 64).slices == 16 && with_chunks(8, 8, 17, 64).slices == 16);
    CHECK(with_chunks(8, 8, 1, 64).chunk[1] == 8);
}

static void test_switches() {
    const char* names[9] = {"KG_NO_SMALL_SELECT", "KG_SMALL_ALLOW_BIG", "KG_SMALL_CHUNKS", "KG_NO_SMALL_FUSED_FINISH",
                            "KG_SMALL_FINISHER", "KG_SMALL_REPLICAS", "KG_SMALL_ROW_RESULTS", "KG_SMALL_PHASES",
                            "KG_PROFILE_BOUND_EVENTS"};
    for (const char* n : names) unsetenv(n);
    SmallSwitches sw = small_switches();
    CHECK(!sw.off && !sw.allow_big && !sw.has_chunks && !sw.no_fused_finish && !sw.finisher && !sw.replicas &&
          !sw.row_results && !sw.phases && !sw.bound_events);
    for (const char* n : names) setenv(n, "1", 1);
    setenv("KG_SMALL_CHUNKS", "7,5,2", 1);
    setenv("KG_SMALL_REPLICAS", "12", 1);
    setenv("KG_SMALL_PHASES", "/tmp/phases.bin", 1);
    sw = small_switches();  // read per call: the same process sees the change
    CHECK(sw.off && sw.allow_big && sw.no_fused_finish && sw.finisher && sw.row_results && sw.bound_events);
    CHECK(sw.has_chunks && sw.chunks[0] == 7 && sw.chunks[1] == 5 && sw.chunks[2] == 2 && sw.replicas == 12);
    CHECK(sw.phases && !std::strcmp(sw.phases, "/tmp/phases.bin"));
    setenv("KG_SMALL_CHUNKS", "7,5", 1);
    setenv("KG_SMALL_REPLICAS", "0", 1);
    setenv("KG_SMALL_PHASES", "", 1);
    sw = small_switches();
    CHECK(!sw.has_chunks && sw.replicas == 0 && !sw.phases);
    setenv("KG_SMALL_REPLICAS", "x", 1);
    CHECK(small_switches().replicas == 0);
    for (const char* n : names) unsetenv(n);
    CHECK(!small_switches().off);
}

// The parity model: a host array plays the two parities; a launch checks that the parity it is handed is all zero,
// zeroes what it was told to zero and dirties its first replicas x lp words.
struct AccModel {
    std::vector<uint8_t> mem = std::vector<uint8_t>(2 * (size_t)SMALL_ACC_SLOTS * 16, 0xEE);  // a new allocation
    AccParity acc;
    uint32_t launches = 0;
    void launch(uint32_t lanes, const SmallSwitches& sw, bool fails) {
        const SmallPlan pl = small_plan(shape(lanes), sw);
        CHECK(pl.take && pl.form == SMALL_ACC);
        const uint32_t slots = pl.replicas * small_lp(lanes);
        CHECK(slots >= 1 && slots <= SMALL_ACC_SLOTS);
        if (acc.clear) {  // ensure_acc
            std::memset(mem.data(), 0, mem.size());
            acc.cleared();
        }
        const AccParity::Next nx = acc.next();
        CHECK(nx.mine != nx.other && nx.mine + nx.other == AccParity::base(1) && nx.zero_n <= SMALL_ACC_SLOTS);
        bool zero = true;
        for (size_t i = 0; i < (size_t)SMALL_ACC_SLOTS * 16; i++) zero = zero && mem[nx.mine + i] == 0;
        CHECK(zero);
        if (fails) {  // half done: some of the zeroing, some of the maxima
            std::memset(mem.data() + nx.other, 0, (size_t)nx.zero_n / 2 * 16);
            std::memset(mem.data() + nx.mine, 0xAB, (size_t)slots / 2 * 16 + 1);
            acc.failed();
        } else {
            std::memset(mem.data() + nx.other, 0, (size_t)nx.zero_n * 16);
            std::memset(mem.data() + nx.mine, 0xAB, (size_t)slots * 16);
            acc.launched(slots);
        }
        launches++;
    }
};

static void test_parity() {
    // test_small_acc_results.py's test_layouts (chunk and replica overrides from call to call, each layout twice and
    // once more behind other forms' selects) and test_shrinking_lane_counts, at 64- and 128-lane shapes
    const struct {
        const char* chunks;
        uint32_t replicas;
    } layouts[] = {{nullptr, 0}, {"8,8,1", 3}, {"7,5,2", 4000}, {"64,64,5", 1}, {"8,8,1", 2}, {nullptr, 0}};
    for (int fail_at = -1; fail_at < 18; fail_at++) {
        AccModel m;
        int step = 0;
        for (uint32_t lanes : {128u, 64u, 100u, 3u})
            for (const auto& l : layouts) {
                SmallSwitches sw;
                sw.replicas = l.replicas;
                if (l.chunks) sw.has_chunks = std::sscanf(l.chunks, "%u,%u,%u", &sw.chunks[0], &sw.chunks[1], &sw.chunks[2]) == 3;
                for (int rep = 0; rep < 3; rep++, step++) m.launch(lanes, sw, step % 19 == fail_at);
            }
        CHECK(m.launches == 72 && !m.acc.clear == (fail_at != 71 % 19));
    }
    AccModel m;
    const SmallSwitches sw;
    for (uint32_t lanes : {256u, 65u, 3u, 256u})
        for (int rep = 0; rep < 3; rep++) m.launch(lanes, sw, lanes == 65 && rep == 1);
    // the invariant itself, after a last launch: 4 replicas x 256 lanes dirty, the other parity clean
    CHECK(m.acc.dirty[m.acc.par] == 0 && m.acc.dirty[m.acc.par ^ 1u] == 4 * 256);
}

static uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

static void test_fold() {
    CHECK(small_status(5, 0) == 0 && small_status(5, 5) == 0 && small_status(5, 6) == KG_ST_UNSUPPORTED);
    CHECK(small_status(0, 0) == 0 && small_status(0, 1) == KG_ST_UNSUPPORTED && small_status(0xFFFFFFFFu, 0xFFFFFFFFu) == 0);
    uint32_t seed = 7;
    for (uint32_t r : {1u, 2u, 4u, 8u})
        for (uint32_t lp : {64u, 256u}) {
            std::vector<uint64_t> stage(SMALL_LRES_WORDS, 0);
            CHECK((size_t)2 * r * lp <= stage.size());
            uint64_t* keys = stage.data();
            uint32_t* fhi = reinterpret_cast<uint32_t*>(keys + (size_t)r * lp);
            uint32_t* ub = fhi + (size_t)r * lp;
            std::vector<uint64_t> want_key(lp);
            std::vector<uint32_t> want_st(lp);
            for (uint32_t j = 0; j < lp; j++) {
                uint64_t k = 0;
                uint32_t f = 0, u = 0;
                for (uint32_t q = 0; q < r; q++) {
                    const size_t at = (size_t)q * lp + j;
                    fhi[at] = lcg(seed) >> 20;
                    keys[at] = ((uint64_t)fhi[at] << 32) | lcg(seed);
                    // lanes j % 4: no unsupported pair, bound == fhi, bound == fhi + 1, anything
                    ub[at] = j % 4 == 0 ? 0u : j % 4 == 3 ? lcg(seed) >> 20 : 0u;
                    k = std::max(k, keys[at]);
                    f = std::max(f, fhi[at]);
                    u = std::max(u, ub[at]);
                }
                if (j % 4 == 1) ub[(size_t)(j % r) * lp + j] = u = f;
                if (j % 4 == 2) ub[(size_t)(j % r) * lp + j] = u = f + 1;
                want_key[j] = k;
                want_st[j] = u != 0 && u > f ? KG_ST_UNSUPPORTED : 0u;
                if (j % 4 == 0 || j % 4 == 1) CHECK(want_st[j] == 0);
                if (j % 4 == 2) CHECK(want_st[j] == KG_ST_UNSUPPORTED);
            }
            LaneResult res;
            res.host = stage.data();
            const uint8_t lane_of[1] = {0};
            res.claim(lp, lane_of, r, nullptr);
            CHECK(res.lanes && !res.fetched && res.fetch_bytes() == (size_t)16 * r * lp);
            res.fold();
            res.fold();  // the second read of the same select folds nothing
            CHECK(res.fetched && res.stat_at == r * lp);
            for (uint32_t j = 0; j < lp; j++) CHECK(res.host[j] == want_key[j] && res.status()[j] == want_st[j]);
            res.reset();
            CHECK(!res.lanes && !res.fetched && res.acc_r == 0 && res.host == stage.data());
            res.claim(lp, lane_of, 0, nullptr);  // LANES: nothing to fold
            CHECK(res.fetch_bytes() == (size_t)12 * lp && res.stat_at == lp);
            res.fold();
            CHECK(res.fetched && res.stat_at == lp && res.host[0] == want_key[0]);
        }
}

int main() {
    test_geometry();
    test_gates_and_forms();
    test_switches();
    test_parity();
    test_fold();
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("small plan ok\n");
    return 0;
}
