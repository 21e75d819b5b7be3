// kg_devmem.h — ownership of device and pinned host buffers in the host runtime.
//
// No HIP include: every allocation goes through the four functions declared below. kg_runtime.cpp defines them as the
// HIP calls and returns the hipError_t; the stand-alone host test (tests/native/devmem_main.cpp) defines them over
// malloc / free. Each returns 0 for success.
#pragma once

#include <cassert>
#include <cstddef>

namespace kg {

int dev_alloc(void** p, size_t bytes);
int dev_free(void* p);
int pinned_alloc(void** p, size_t bytes);
int pinned_free(void* p);

struct DevMem {
    static int alloc(void** p, size_t bytes) { return dev_alloc(p, bytes); }
    static int free(void* p) { return dev_free(p); }
};
struct PinnedMem {
    static int alloc(void** p, size_t bytes) { return pinned_alloc(p, bytes); }
    static int free(void* p) { return pinned_free(p); }
};

// One allocation of cap() elements of T. Move-only; the destructor frees. Converts to T*, so reading sites use it like
// the raw pointer. Sizes are exact: floors and spare slots are the caller's.
template <class T, class Mem>
class Buf {
public:
    Buf() = default;
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    Buf(Buf&& o) noexcept : p_(o.p_), cap_(o.cap_) {
        o.p_ = nullptr;
        o.cap_ = 0;
    }
    Buf& operator=(Buf&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = o.p_;
            cap_ = o.cap_;
            o.p_ = nullptr;
            o.cap_ = 0;
        }
        return *this;
    }
    ~Buf() { reset(); }

    operator T*() const { return p_; }
    T* get() const { return p_; }
    size_t cap() const { return cap_; }

    // n elements into an empty buffer
    int alloc(size_t n) {
        assert(!p_ && !cap_);
        void* v = nullptr;
        const int e = Mem::alloc(&v, sizeof(T) * n);
        if (e != 0) return e;
        p_ = static_cast<T*>(v);
        cap_ = n;
        return 0;
    }
    // At least n elements; the contents are not kept. After a failure the buffer is empty, so the next call allocates again.
    int reserve(size_t n) {
        if (cap_ >= n) return 0;
        const int e = reset();
        return e != 0 ? e : alloc(n);
    }
    int reset() {
        T* p = p_;
        p_ = nullptr;
        cap_ = 0;
        return p ? Mem::free(p) : 0;
    }

private:
    T* p_ = nullptr;
    size_t cap_ = 0;
};

template <class T>
using DevBuf = Buf<T, DevMem>;
template <class T>
using PinnedBuf = Buf<T, PinnedMem>;

}  // namespace kg
