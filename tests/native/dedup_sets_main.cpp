// Stand-alone check of kg_dedup.h with candidate node sets: the set id counted into the row, and the split of a lane
// list into the lanes without a set (order kept) and the lanes with one (sorted by set, fast before integer lanes, wave
// kind). Built with the host compiler and -fsanitize=address,undefined by tests/test_node_sets_host.py; exits non-zero
// on the first failed check.
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

template <class Hash>
void run_cases() {
    const uint32_t n = 96;
    std::vector<int64_t> col[DEDUP_COLS];
    for (auto& c : col) c.assign(n, 5);
    std::vector<uint32_t> flags(n, 0x10003u);
    std::vector<int32_t> set(n);
    std::vector<uint8_t> kind(n);
    for (uint32_t j = 0; j < n; j++) {
        col[0][j] = j % 4;                 // 4 distinct rows
        kind[j] = (uint8_t)(j % 4);        // one wave kind per row; kind 3 = integer lane
        set[j] = (int32_t)(j / 4 % 3) - 1; // -1, 0, 1 in turn: every row meets every set
    }
    DedupRows rows{};
    for (int c = 0; c < DEDUP_COLS; c++) rows.col[c] = col[c].data();
    rows.flags = flags.data();
    std::vector<uint32_t> rep(n, 0xDEADBEEFu), slots;
    // without the set column: 4 representatives
    CHECK(dedup_rows(rows, n, rep.data(), slots, Hash()) == 4);
    for (uint32_t j = 0; j < n; j++) CHECK(rep[j] == j % 4);
    // with it: 4 rows x 3 sets, each the lowest equal (row, set)
    rows.set = set.data();
    CHECK(dedup_rows(rows, n, rep.data(), slots, Hash()) == 12);
    for (uint32_t j = 0; j < n; j++) CHECK(rep[j] == j % 12);
    CHECK(!dedup_row_equal(rows, 0, 4) && dedup_row_equal(rows, 0, 12));

    // lane lists: fast lanes grouped by wave kind, then the integer lanes
    std::vector<uint32_t> order;
    for (uint32_t k = 0; k < 4; k++)
        for (uint32_t j = 0; j < n; j++)
            if (kind[j] == k) order.push_back(j);
    const uint32_t n_fast = n / 4 * 3;
    std::vector<uint32_t> rorder(n, 0xDEADBEEFu);
    uint32_t nrf = 0, nr = 0;
    dedup_order(order.data(), n, n_fast, rep.data(), rorder.data(), &nrf, &nr);
    CHECK(nr == 12 && nrf == 9);
    // split of the representatives: buffers exactly as long as the lists (a write past them is an ASan report)
    std::vector<uint32_t> list(rorder.begin(), rorder.begin() + nr), set_list(nr, 0xDEADBEEFu);
    uint32_t plain = 0, plain_fast = 0;
    const uint32_t ns = dedup_split_sets(list.data(), nr, nrf, set.data(), kind.data(), set_list.data(), &plain, &plain_fast);
    CHECK(ns == 8 && plain == 4 && plain_fast == 3);
    for (uint32_t t = 0; t < plain; t++) CHECK(set[list[t]] == -1 && kind[list[t]] == t);  // order kept
    for (uint32_t t = 0; t < ns; t++) {
        CHECK(set[set_list[t]] == (int32_t)(t / 4));  // sorted by set
        CHECK(kind[set_list[t]] == t % 4);            // then fast lanes by wave kind, the integer lane last
    }
    // split of the full list
    std::vector<uint32_t> full(order), full_sets(n, 0xDEADBEEFu);
    const uint32_t nfs = dedup_split_sets(full.data(), n, n_fast, set.data(), kind.data(), full_sets.data(), &plain, &plain_fast);
    CHECK(nfs == 64 && plain == 32 && plain_fast == 24);
    for (uint32_t t = 1; t < nfs; t++) {
        const uint32_t a = full_sets[t - 1], b = full_sets[t];
        CHECK(set[a] < set[b] || (set[a] == set[b] && kind[a] <= kind[b]));
    }
    for (uint32_t t = 0; t < plain; t++) CHECK(set[full[t]] == -1 && (t < plain_fast) == (kind[full[t]] < 3));
    // no set lanes, and no lanes
    std::vector<int32_t> none(n, -1);
    std::vector<uint32_t> again(order);
    CHECK(dedup_split_sets(again.data(), n, n_fast, none.data(), kind.data(), full_sets.data(), &plain, &plain_fast) == 0);
    CHECK(plain == n && plain_fast == n_fast && again == order);
    CHECK(dedup_split_sets(again.data(), 0, 0, none.data(), kind.data(), full_sets.data(), &plain, &plain_fast) == 0);
    CHECK(plain == 0 && plain_fast == 0);
}

}  // namespace

int main() {
    run_cases<DedupHash>();
    run_cases<ConstHash>();
    if (failures) {
        std::fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    std::puts("dedup sets ok");
    return 0;
}
