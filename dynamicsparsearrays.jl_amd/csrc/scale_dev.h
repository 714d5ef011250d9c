// csrc/scale_dev.h — the span shape of the streaming passes over the stored values, shared by scale.hip (reduce, scale) and
// droptol.hip (the decide pass of dropzeros! / droptol!): one wave per span of 512 slots (8 occupancy words), four independent waves
// per workgroup; the span's occupancy words, keys and values requested at once; the lane helpers of the owner lookup (the nearest
// semaphore at or below a lane); and the layout of the scale scratch.  Device code, and the host-side carve of that scratch.
#pragma once
#include "wave_dev.h"
#include <type_traits>

namespace dsa {

constexpr int SC_BLOCK = 256;
constexpr int SC_WAVES = SC_BLOCK / 64;
constexpr int SC_WORDS = 8;                               // occupancy words of a span
constexpr int64_t SC_SPAN = SC_WORDS * 64;                // slots of a span

// scratch layout: 16 header bytes {error word, ticket, pad, pad}, then arrays of one 8-byte entry per span
struct ScHeader { uint32_t err, ticket, pad0, pad1; };
static inline int64_t sc_spans(int64_t capacity) { return (((capacity + 63) >> 6) + SC_WORDS - 1) / SC_WORDS; }

struct ScScratch {
    ScHeader* hdr; int64_t nspans; void* a0; void* a1; void* a2;
    ScScratch(void* scratch, int64_t capacity) : hdr(static_cast<ScHeader*>(scratch)), nspans(sc_spans(capacity)) {
        char* p = static_cast<char*>(scratch) + sizeof(ScHeader);
        a0 = p; a1 = p + (size_t)nspans * 8; a2 = p + (size_t)nspans * 16;
    }
};

__device__ __forceinline__ uint64_t mask_le(int i) { return mask_lt(i + 1); }                     // bits [0, i]
__device__ __forceinline__ int top_bit(uint64_t x) { return 63 - __clzll((long long)x); }         // x != 0
__device__ __forceinline__ double readlane_f64(double v, int l) { return __longlong_as_double((long long)readlane64((uint64_t)__double_as_longlong(v), l)); }

// the span of this wave: its occupancy words (wave-uniform; words behind the array are empty), keys and values, all requested at once
template <bool WIDE, bool NT, bool VALS>
__device__ __forceinline__ void sc_load_span(const typename std::conditional<WIDE, int64_t, int32_t>::type* __restrict__ kp,
                                             const double* __restrict__ vals, const uint64_t* __restrict__ occ, int64_t nwords, int64_t w0,
                                             int lane, uint64_t (&ow)[SC_WORDS], typename std::conditional<WIDE, int64_t, int32_t>::type (&k)[SC_WORDS],
                                             double (&v)[SC_WORDS]) {
#pragma unroll
    for (int j = 0; j < SC_WORDS; ++j) ow[j] = occ[w0 + j < nwords ? w0 + j : nwords - 1];
#pragma unroll
    for (int j = 0; j < SC_WORDS; ++j) {
        const int64_t w = w0 + j < nwords ? w0 + j : nwords - 1;          // slot buffers are allocated in whole words
        k[j] = NT ? __builtin_nontemporal_load(kp + (w << 6) + lane) : kp[(w << 6) + lane];
    }
    if (VALS) {
#pragma unroll
        for (int j = 0; j < SC_WORDS; ++j) {
            const int64_t w = w0 + j < nwords ? w0 + j : nwords - 1;
            v[j] = NT ? __builtin_nontemporal_load(vals + (w << 6) + lane) : vals[(w << 6) + lane];
        }
    }
#pragma unroll
    for (int j = 0; j < SC_WORDS; ++j) ow[j] = w0 + j < nwords ? readfirstlane64(ow[j]) : 0ull;
}

}  // namespace dsa
