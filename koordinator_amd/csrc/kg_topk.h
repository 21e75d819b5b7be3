// kg_topk.h — per-lane top-K lists of packed selection keys and their insertion into a pod's shared slots (device
// only; shared by the select kernels of kg_kernels.hip and kg_sets.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "kg_layout.h"

namespace kg {

template <int K>
__device__ __forceinline__ void topk_insert(uint64_t (&top)[K], uint64_t key) {
    if constexpr (K == 1) {
        top[0] = key > top[0] ? key : top[0];
    } else {
        // a wave-uniform skip when no lane's key enters its top-K (most records once the lists have filled): the
        // cascade below leaves top unchanged for a key not above top[K-1], so the lanes that do not insert may run it
        if (!__any(key > top[K - 1])) return;
#pragma unroll
        for (int t = 0; t < K; t++) {
            const uint64_t cur = top[t];
            const bool gt = key > cur;
            top[t] = gt ? key : cur;
            key = gt ? cur : key;
        }
    }
}

// Insert a lane's top-K (descending, zeros = none) into the K shared slots of its pod, out[0..K), by an
// atomicMax cascade: each key goes down the slots, an atomicMax at slot u keeps the larger of (slot, key) and
// the smaller continues to slot u + 1. Whatever the interleaving of the lanes (chunks) that insert into one
// pod, slot u ends as the u-th largest key inserted (the values passed below slot u are exactly its arrivals
// minus their maximum), and slot u >= slot u + 1 at every instant; slots only grow. So a key that is not
// above slot K-1 (read once, a lower bound of every slot from then on) can stop.
template <int K>
__device__ __forceinline__ void topk_atomic(uint64_t* out, const uint64_t (&top)[K]) {
    if (top[0] == 0ull) return;
    const uint64_t floor = __hip_atomic_load(out + (K - 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
    for (int t = 0; t < K; t++) {
        uint64_t carry = top[t];
        if (carry <= floor) break;  // top is descending: every later key stops too
#pragma unroll
        for (int u = 0; u < K; u++) {
            if (carry <= floor) break;
            const uint64_t old = atomicMax((unsigned long long*)(out + u), (unsigned long long)carry);
            carry = old < carry ? old : carry;
        }
    }
}

__device__ __forceinline__ uint32_t rec_gidx(const NodeRec& r, uint32_t index_base) {
    return index_base + node_index(r);
}

}  // namespace kg
