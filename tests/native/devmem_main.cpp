// Stand-alone check of kg_devmem.h (owning device / pinned buffers of the host runtime). Defines the four allocation
// functions over malloc / free with a live-allocation count and a "fail the N-th allocation" switch. Built with the host
// compiler and -fsanitize=address,undefined by tests/test_devmem_host.py; exits non-zero on the first failed check.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <utility>

#include "../../koordinator_amd/csrc/kg_devmem.h"

namespace {

int failures = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                     \
        }                                                                   \
    } while (0)

int live = 0;         // allocations not yet freed (device and pinned)
int allocs = 0;       // allocations attempted since the last arm()
int fail_at = 0;      // the allocation (1-based) that fails, 0 = none
size_t last_bytes = 0;

void arm(int nth) {
    allocs = 0;
    fail_at = nth;
}

int test_alloc(void** p, size_t bytes) {
    last_bytes = bytes;
    if (++allocs == fail_at) return 2;  // hipErrorOutOfMemory's value; any non-zero code serves
    *p = std::malloc(bytes ? bytes : 1);
    if (!*p) return 2;
    live++;
    return 0;
}

int test_free(void* p) {
    std::free(p);
    live--;
    return 0;
}

}  // namespace

int kg::dev_alloc(void** p, size_t bytes) { return test_alloc(p, bytes); }
int kg::dev_free(void* p) { return test_free(p); }
int kg::pinned_alloc(void** p, size_t bytes) { return test_alloc(p, bytes); }
int kg::pinned_free(void* p) { return test_free(p); }

using namespace kg;

namespace {

void test_alloc_reserve() {
    arm(0);
    {
        DevBuf<uint64_t> b;
        CHECK(b == nullptr && b.cap() == 0);
        CHECK(b.alloc(10) == 0);
        uint64_t* p0 = b;
        CHECK(p0 != nullptr && b.cap() == 10 && last_bytes == 80 && live == 1);
        p0[9] = 7;  // the last element is inside the allocation
        CHECK(b.reserve(4) == 0);  // smaller: nothing happens
        CHECK(b == p0 && b.cap() == 10 && allocs == 1);
        CHECK(b.reserve(10) == 0);  // equal: nothing happens
        CHECK(b == p0 && b.cap() == 10 && allocs == 1);
        CHECK(b.reserve(11) == 0);  // larger: a fresh allocation of exactly 11
        CHECK(b != nullptr && b.cap() == 11 && last_bytes == 88 && allocs == 2 && live == 1);
        b[10] = 9;
        CHECK(b + 1 == &b[1]);  // reads like the raw pointer
        DevBuf<uint8_t> e;
        CHECK(e.reserve(0) == 0);  // nothing to do for an empty request
        CHECK(!e && e.cap() == 0 && allocs == 2);
    }
    CHECK(live == 0);
}

void test_move() {
    arm(0);
    {
        DevBuf<uint32_t> a;
        CHECK(a.alloc(3) == 0);
        uint32_t* pa = a;
        DevBuf<uint32_t> b(std::move(a));
        CHECK(b == pa && b.cap() == 3 && a == nullptr && a.cap() == 0 && live == 1);
        DevBuf<uint32_t> c;
        CHECK(c.alloc(5) == 0);
        CHECK(live == 2);
        c = std::move(b);  // frees c's old buffer
        CHECK(c == pa && c.cap() == 3 && b == nullptr && b.cap() == 0 && live == 1);
        DevBuf<uint32_t>& self = c;
        c = std::move(self);
        CHECK(c == pa && c.cap() == 3 && live == 1);
        PinnedBuf<uint8_t> h;
        CHECK(h.alloc(16) == 0 && h.cap() == 16 && live == 2);
        PinnedBuf<uint8_t> h2 = std::move(h);
        CHECK(h2 != nullptr && !h && live == 2);
    }
    CHECK(live == 0);
}

void test_reset() {
    arm(0);
    DevBuf<int32_t> b;
    CHECK(b.alloc(8) == 0 && live == 1);
    CHECK(b.reset() == 0);
    CHECK(b == nullptr && b.cap() == 0 && live == 0);
    CHECK(b.reset() == 0);
    CHECK(b == nullptr && b.cap() == 0 && live == 0);
    CHECK(b.alloc(2) == 0 && b.cap() == 2);  // empty again: alloc is allowed
    b.reset();
    CHECK(live == 0);
}

// kg_snapshot_create: six buffers allocated in one chain, the object deleted on failure
struct Six {
    DevBuf<uint64_t> a, b;
    DevBuf<uint32_t> c;
    DevBuf<int8_t> d;
    DevBuf<int32_t> e;
    DevBuf<uint32_t> f;
    bool create(size_t n) {
        return !(a.alloc(n) || b.alloc(n) || c.alloc(n + 1) || d.alloc(2 * n) || e.alloc(2 * n) || f.alloc(n));
    }
};

void test_six() {
    for (int nth : {1, 3, 6}) {
        arm(nth);
        Six* s = new Six();
        CHECK(!s->create(100));
        CHECK(live == nth - 1 && allocs == nth);
        delete s;
        CHECK(live == 0);
    }
    arm(0);
    Six* s = new Six();
    CHECK(s->create(100) && live == 6);
    delete s;
    CHECK(live == 0);
}

// d_ipairs + d_ipair_count: one logical capacity, set once both buffers stand
struct Group {
    DevBuf<uint32_t> x, y;
    size_t cap = 0;
    int ensure(size_t n) {
        if (n <= cap) return 0;
        cap = 0;
        if (int e = x.reserve(4 * n)) return e;
        if (int e = y.reserve(n)) return e;
        cap = n;
        return 0;
    }
};

void test_group() {
    arm(0);
    {
        Group g;
        CHECK(g.ensure(64) == 0 && g.cap == 64 && live == 2);
        arm(2);  // the second buffer's allocation fails
        CHECK(g.ensure(200) != 0);
        CHECK(g.cap == 0 && g.x.cap() == 800 && g.y == nullptr && g.y.cap() == 0 && live == 1);
        arm(0);
        CHECK(g.ensure(200) == 0);  // the retry allocates what is missing
        CHECK(g.cap == 200 && g.x.cap() == 800 && g.y.cap() == 200 && g.y != nullptr && live == 2 && allocs == 1);
        arm(1);  // the first buffer's allocation fails: the retry allocates both
        CHECK(g.ensure(300) != 0);
        CHECK(g.cap == 0 && g.x == nullptr && g.x.cap() == 0 && g.y.cap() == 200 && live == 1);
        arm(0);
        CHECK(g.ensure(300) == 0);
        CHECK(g.cap == 300 && g.x.cap() == 1200 && g.y.cap() == 300 && live == 2 && allocs == 2);
    }
    CHECK(live == 0);
}

void test_failed_reserve() {
    arm(0);
    DevBuf<uint64_t> b;
    CHECK(b.alloc(4) == 0 && live == 1);
    arm(1);
    CHECK(b.reserve(5) != 0);
    CHECK(b == nullptr && b.cap() == 0 && live == 0);  // empty, never half-described
    arm(0);
    CHECK(b.reserve(5) == 0 && b != nullptr && b.cap() == 5 && live == 1);
    arm(1);
    DevBuf<uint64_t> c;
    CHECK(c.alloc(3) != 0);
    CHECK(c == nullptr && c.cap() == 0);
    arm(0);
}

}  // namespace

int main() {
    test_alloc_reserve();
    test_move();
    test_reset();
    test_six();
    test_group();
    test_failed_reserve();
    CHECK(live == 0);
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("devmem ok\n");
    return 0;
}
