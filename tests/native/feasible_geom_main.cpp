// Stand-alone check of the launch geometry of kg_feasible.h (the lane = row form of kg_eval_feasible's step 1): chunk
// starts are multiples of 64 records, so every 64-bit word of the record-order bitmap has one writer, and the chunks of
// all launches cover every record once. Built with the host compiler and -fsanitize=address,undefined by
// tests/test_feasible_host.py; exits non-zero on the first failed check.
#include <algorithm>
#include <cstdio>
#include <vector>

#define KG_FEASIBLE_GEOMETRY_ONLY
#include "../../koordinator_amd/csrc/kg_feasible.h"

using namespace kg;

namespace {

int failures = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                     \
        }                                                                   \
    } while (0)

// The launcher's loops (launch_feasible_records, lane = row form), writers counted per word.
void walk(uint32_t n_nodes, uint32_t n_rows, uint32_t target) {
    const uint32_t block = std::min<uint32_t>(256u, (n_rows + 63u) / 64u * 64u);
    const uint32_t chunk = feasible_chunk(n_nodes, n_rows, block, target);
    CHECK(chunk >= 64u && chunk % 64u == 0u);
    CHECK(feasible_span(chunk) % 64u == 0u);
    std::vector<uint32_t> writers(feasible_words(n_nodes), 0u);
    uint64_t records = 0;
    for (uint64_t begin = 0; begin < n_nodes; begin += feasible_span(chunk)) {
        const uint32_t end = (uint32_t)std::min<uint64_t>(n_nodes, begin + feasible_span(chunk));
        const uint32_t gy = (end - (uint32_t)begin + chunk - 1u) / chunk;
        CHECK(gy >= 1u && gy <= FEAS_MAX_Y);
        for (uint32_t y = 0; y < gy; y++) {
            const uint32_t lo = (uint32_t)begin + y * chunk, hi = std::min(end, lo + chunk);
            CHECK(lo % 64u == 0u && lo < hi);
            for (uint32_t w0 = lo; w0 < hi; w0 += 64u) {
                CHECK((w0 >> 6) < writers.size());
                if ((w0 >> 6) < writers.size()) writers[w0 >> 6]++;
            }
            records += hi - lo;
        }
    }
    CHECK(records == n_nodes);
    for (uint32_t w : writers) CHECK(w == 1u);
}

}  // namespace

int main() {
    CHECK(feasible_words32(0) == 0u && feasible_words32(1) == 1u && feasible_words32(32) == 1u && feasible_words32(33) == 2u);
    CHECK(feasible_words(0) == 0u && feasible_words(64) == 1u && feasible_words(65) == 2u);
    for (uint32_t n : {1u, 63u, 64u, 65u, 100000u})
        for (uint32_t rows : {1u, 8u, 64u, 100u, 1000u, 10000u})
            for (uint32_t target : {1u, 7u, FEAS_TARGET_BLOCKS, 65536u}) walk(n, rows, target);
    // a snapshot past one launch's span: 64-record chunks (a large target) over 5 million records
    walk(5000000u, 1u, 1u << 20);
    CHECK(feasible_chunk(5000000u, 1u, 64u, 1u << 20) == 64u);
    CHECK(feasible_chunk(100000u, 1u, 64u) == 64u && feasible_chunk(10000u, 10000u, 256u) == 256u);
    // the form rule: enough pairs and at least half a wave of rows for lane = row
    CHECK(feasible_rows_form(10000u, 10000u) && feasible_rows_form(32u, 100000u) && feasible_rows_form(1000u, 10000u));
    CHECK(!feasible_rows_form(1u, 100000u) && !feasible_rows_form(100u, 10000u) && !feasible_rows_form(16u, 1000000u));
    CHECK(feasible_rows_form(0xFFFFFFFFu, 0xFFFFFFFFu) && !feasible_rows_form(0u, 0u));
    if (failures) return 1;
    std::printf("feasible geometry ok\n");
    return 0;
}
