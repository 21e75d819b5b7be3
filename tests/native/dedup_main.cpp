// Stand-alone check of kg_dedup.h (representative rows of a pod batch). Built with the host compiler and
// -fsanitize=address,undefined by tests/test_pod_dedup_host.py; exits non-zero on the first failed check.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../koordinator_amd/csrc/kg_dedup.h"

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

struct ConstHash {  // every row collides
    uint64_t operator()(const DedupRows&, uint32_t) const { return 7; }
};

struct Batch {
    uint32_t n;
    std::vector<int64_t> col[DEDUP_COLS];
    std::vector<uint32_t> flags;
    explicit Batch(uint32_t n_) : n(n_), flags(n_, 0x10003u) {
        for (auto& c : col) c.assign(n_, 5);
    }
    DedupRows rows() const {
        DedupRows r{};
        for (int c = 0; c < DEDUP_COLS; c++) r.col[c] = col[c].data();
        r.flags = flags.data();
        return r;
    }
};

// brute force: the lowest equal row
std::vector<uint32_t> want_rep(const Batch& b, uint32_t n) {
    const DedupRows r = b.rows();
    std::vector<uint32_t> w(n);
    for (uint32_t j = 0; j < n; j++) {
        w[j] = j;
        for (uint32_t i = 0; i < j; i++)
            if (dedup_row_equal(r, i, j)) {
                w[j] = i;
                break;
            }
    }
    return w;
}

template <class Hash>
void check(const Batch& b, uint32_t n, std::vector<uint32_t>& rep, std::vector<uint32_t>& slots, uint32_t want_n_rep) {
    // buffers are exactly n long: a write past row n is an ASan report
    std::vector<uint32_t> out(n, 0xDEADBEEFu);
    const uint32_t got = dedup_rows(b.rows(), n, out.data(), slots, Hash());
    const std::vector<uint32_t> want = want_rep(b, n);
    CHECK(got == want_n_rep);
    CHECK(out == want);
    rep = out;
}

template <class Hash>
void run_cases() {
    std::vector<uint32_t> rep, slots;
    {  // n = 0 and n = 1
        Batch b(1);
        check<Hash>(b, 0, rep, slots, 0);
        check<Hash>(b, 1, rep, slots, 1);
        CHECK(rep[0] == 0);
    }
    {  // all rows equal
        Batch b(300);
        check<Hash>(b, 300, rep, slots, 1);
        for (uint32_t j = 0; j < 300; j++) CHECK(rep[j] == 0);
    }
    {  // all rows distinct
        Batch b(300);
        for (uint32_t j = 0; j < 300; j++) b.col[2][j] = j;
        check<Hash>(b, 300, rep, slots, 300);
        for (uint32_t j = 0; j < 300; j++) CHECK(rep[j] == j);
    }
    // rows that differ in one column only: each int64 column (low and high bits), then the flags word's KG_POD_* bits,
    // its NUMA-policy bits (<< 16) and a high bit (POD_FASTV's region)
    for (int c = 0; c < DEDUP_COLS; c++)
        for (int64_t delta : {(int64_t)1, (int64_t)1 << 40, (int64_t)-6}) {
            Batch b(64);
            for (uint32_t j = 1; j < 64; j += 2) b.col[c][j] += delta;
            check<Hash>(b, 64, rep, slots, 2);
            for (uint32_t j = 0; j < 64; j++) CHECK(rep[j] == (j & 1u));
        }
    for (uint32_t bit : {1u << 2, 1u << 16, 3u << 16, 1u << 30}) {
        Batch b(64);
        for (uint32_t j = 1; j < 64; j += 2) b.flags[j] ^= bit;
        check<Hash>(b, 64, rep, slots, 2);
        for (uint32_t j = 0; j < 64; j++) CHECK(rep[j] == (j & 1u));
    }
    {  // values swapped between two columns are different rows
        Batch b(2);
        b.col[0][0] = 1, b.col[1][0] = 2;
        b.col[0][1] = 2, b.col[1][1] = 1;
        check<Hash>(b, 2, rep, slots, 2);
    }
    {  // a second call with a smaller n into the same buffers: nothing of the first call survives
        Batch b(200);
        for (uint32_t j = 0; j < 200; j++) b.col[4][j] = j % 50;
        std::vector<uint32_t> out(200), slots2;
        CHECK(dedup_rows(b.rows(), 200, out.data(), slots2, Hash()) == 50);
        for (uint32_t j = 0; j < 200; j++) b.col[4][j] = j % 3;
        for (uint32_t j = 40; j < 200; j++) out[j] = 0xDEADBEEFu;
        CHECK(dedup_rows(b.rows(), 40, out.data(), slots2, Hash()) == 3);
        for (uint32_t j = 0; j < 40; j++) CHECK(out[j] == j % 3);
        for (uint32_t j = 40; j < 200; j++) CHECK(out[j] == 0xDEADBEEFu);
    }
    {  // lane lists: grouping kept, first occurrence not first of its group, duplicates across the kinds
        // rows: kind by j % 4 (3 = integer lane), value j % 8 -> 8 distinct rows, representatives 0..7
        const uint32_t n = 40;
        Batch b(n);
        std::vector<uint32_t> kind(n);
        for (uint32_t j = 0; j < n; j++) {
            kind[j] = j % 4;
            b.col[0][j] = j % 8;
        }
        std::vector<uint32_t> order, out(n);
        for (uint32_t k = 0; k < 4; k++)
            for (uint32_t j = 0; j < n; j++)
                if (kind[j] == k) order.push_back(j);
        const uint32_t n_fast = 30;
        CHECK(dedup_rows(b.rows(), n, out.data(), slots, Hash()) == 8);
        std::vector<uint32_t> rorder(n, 0xDEADBEEFu);
        uint32_t nrf = 0, nr = 0;
        dedup_order(order.data(), n, n_fast, out.data(), rorder.data(), &nrf, &nr);
        CHECK(nr == 8 && nrf == 6);
        const uint32_t want[8] = {0, 4, 1, 5, 2, 6, 3, 7};
        for (uint32_t t = 0; t < 8; t++) CHECK(rorder[t] == want[t]);
        CHECK(rorder[8] == 0xDEADBEEFu);
        // no fast lanes at all, and no lanes
        dedup_order(order.data(), n, 0, out.data(), rorder.data(), &nrf, &nr);
        CHECK(nr == 8 && nrf == 0);
        dedup_order(order.data(), 0, 0, out.data(), rorder.data(), &nrf, &nr);
        CHECK(nr == 0 && nrf == 0);
    }
    CHECK(dedup_waves(0, 0) == 0 && dedup_waves(64, 64) == 1 && dedup_waves(66, 65) == 3 && dedup_waves(130, 0) == 3);
}

}  // namespace

int main() {
    run_cases<DedupHash>();
    run_cases<ConstHash>();
    if (failures) {
        std::fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    std::puts("dedup ok");
    return 0;
}
