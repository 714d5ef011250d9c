// csrc/wave_dev.h — the wave-level primitives and the pinned hand-over that more than one kernel unit uses.  Device code only: a
// kernel unit includes it, a host unit never does.  A wave is 64 lanes; every function here is called by a whole wave (the
// hand-over by the one thread that publishes, the bisection by one thread).
#pragma once
#include "dsa_dev.h"

namespace dsa {

// ---- reductions over the wave (xor butterfly, o = 32 .. 1: the order of the double version decides the bits of an SpMV result)
__device__ __forceinline__ uint32_t wave_reduce_add(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int64_t wave_reduce_add(int64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_reduce_add(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ uint32_t wave_or(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v |= (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const uint32_t y = __shfl_xor(v, o, 64); v = y > v ? y : v; }
    return v;
}
// sum of v over the lanes in front of this one
__device__ __forceinline__ uint32_t wave_excl_scan(uint32_t v) {
    const int lane = lane_id();
    uint32_t x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    return x - v;
}

// ---- a value of lane l / of the first active lane, as a wave-uniform value: 32 bits (int or uint32_t, the type is kept), 64 bits
template <typename T> __device__ __forceinline__ T readlane32(T v, int l) {
    static_assert(sizeof(T) == 4, "one register");
    return (T)__builtin_amdgcn_readlane((int)v, l);
}
template <typename T> __device__ __forceinline__ T readfirstlane32(T v) {
    static_assert(sizeof(T) == 4, "one register");
    return (T)__builtin_amdgcn_readfirstlane((int)v);
}
__device__ __forceinline__ uint64_t readlane64(uint64_t v, int l) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t readfirstlane64(uint64_t w) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)w);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(w >> 32));
    return ((uint64_t)hi << 32) | lo;
}

// ---- bisection over a packed key stream (ascending, distinct keys: the output of K-pack): the first index whose key is >= `key`
// (upper: > `key`), n when there is none.  One thread, log2(n) dependent loads.  The merge of k_merge_axpby (rebalance.hip) and the
// lookups of the dot product (vecops.hip) share it.
__device__ __forceinline__ int64_t packed_bound(KeyArr k, int64_t n, int64_t key, bool upper) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        const int64_t c = k[mid];
        if (c < key || (upper && c == key)) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// ---- the pinned hand-over: a result goes to PINNED HOST memory without a copy command, an event or a stream sync.  The publishing
// thread writes the payload words with relaxed system-scope stores, then calls publish_seq on the sequence word the host polls
// for (host.h: wait_handover): the release fence orders every payload store in front of the sequence number.
__device__ __forceinline__ void publish_seq(unsigned long long* word, unsigned long long seq) {
    __atomic_thread_fence(__ATOMIC_RELEASE);
    __hip_atomic_store(word, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

}  // namespace dsa
