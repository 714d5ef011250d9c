// csrc/export_dev.h — what the export kernel units share (compress.hip: the whole orientation, select.hip: the partitions of
// a key list, submatrix.hip: those partitions restricted to an inner key list): the tile they cut the slot array into, the block
// scan between their count and emit launches, the span of an outer key (select.hip, submatrix.hip) and the end of an emit kernel.
// Device code only.
#pragma once
#include "wave_dev.h"
#include "find_dev.h"

namespace dsa {

constexpr int EX_TILE_SHIFT = 11;                        // 2048 slots = 32 bitmap words: one wave (8192 waves for 2^24 slots)
constexpr int64_t EX_TILE = int64_t(1) << EX_TILE_SHIFT;
constexpr int EX_WORDS = (int)(EX_TILE >> 6);
constexpr int EX_U = 8;                                  // bitmap words whose keys and values a wave requests at once
constexpr int EX_SCAN_THREADS = 1024;

// One workgroup of EX_SCAN_THREADS: exclusive prefixes of a[0..n) and b[0..n), 8192 entries per step, the sums of the steps in
// front carried along.  put(i, pa, pb) gets the two prefixes of entry i (it may overwrite a[i] and b[i]); the totals come back in
// tot_a / tot_b, the same in every thread.
template <typename T, typename Put>
__device__ __forceinline__ void block_excl_scan2(const T* a, const T* b, int64_t n, Put put, unsigned long long& tot_a,
                                                 unsigned long long& tot_b) {
    __shared__ unsigned long long sO[EX_SCAN_THREADS], sS[EX_SCAN_THREADS];
    const int t = threadIdx.x;
    constexpr int PER = 8;
    unsigned long long carry_o = 0, carry_s = 0;
    for (int64_t c0 = 0; c0 < n; c0 += (int64_t)EX_SCAN_THREADS * PER) {
        unsigned long long vo[PER], vs[PER], to = 0, ts = 0;
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const int64_t i = c0 + (int64_t)t * PER + q;
            vo[q] = i < n ? (unsigned long long)a[i] : 0ull;
            vs[q] = i < n ? (unsigned long long)b[i] : 0ull;
            to += vo[q]; ts += vs[q];
        }
        sO[t] = to; sS[t] = ts;
        __syncthreads();
        for (int o = 1; o < EX_SCAN_THREADS; o <<= 1) {          // inclusive scan (Hillis-Steele)
            const unsigned long long x = t >= o ? sO[t - o] : 0ull, y = t >= o ? sS[t - o] : 0ull;
            __syncthreads();
            sO[t] += x; sS[t] += y;
            __syncthreads();
        }
        unsigned long long ro = carry_o + sO[t] - to, rs = carry_s + sS[t] - ts;
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const int64_t i = c0 + (int64_t)t * PER + q;
            if (i < n) put(i, ro, rs);
            ro += vo[q]; rs += vs[q];
        }
        carry_o += sO[EX_SCAN_THREADS - 1]; carry_s += sS[EX_SCAN_THREADS - 1];
        __syncthreads();
    }
    tot_a = carry_o; tot_b = carry_s;
}

// occupied slots of [from, to) (0-based, from < to): the lanes stride over the words, first and last word masked
__device__ __forceinline__ int64_t sel_span_popc(const uint64_t* __restrict__ occ, int64_t from, int64_t to, int lane) {
    int64_t c = 0;
    const int64_t w1 = (to - 1) >> 6;
    for (int64_t w = (from >> 6) + lane; w <= w1; w += 64) c += popc64(occ[w] & word_range_mask(w, from, to - 1));
    return wave_reduce_add(c);
}

// The span of the live partition whose key is `key` (one wave, the same answer in every lane): its cells are the occupied slots of
// [lo, hi), 0-based, strictly between its semaphore and the next live semaphore (tombstoned table entries behind the partition are
// skipped 64 at a time; the end of the slot array behind the last one).  lo = hi = 0 for a key without a live partition.
// err: 1 the key lies outside 1..dim_out, 2 tables out of step with the slots.
struct KeySpan { int64_t lo, hi; uint32_t err; };
__device__ __forceinline__ KeySpan key_span(int64_t capacity, const int64_t* __restrict__ sems, const int64_t* __restrict__ col_keys,
                                            const uint8_t* __restrict__ col_live, int64_t table_len, bool dense, int64_t key,
                                            int64_t dim_out, int lane) {
    KeySpan r{0, 0, 0u};
    if (key < 1 || key > dim_out) {
        r.err = 1u;
    } else {
        const DFoundKey f = d_find_table_fast(col_keys, col_live, table_len, key, dense);
        if (f.has && f.key == key) {
            const int64_t sp = sems[f.pos - 1];                  // 1-based slot of the semaphore = 0-based slot of the first cell
            int64_t nx = 0;                                      // the next live semaphore (tombstones have none)
            for (int64_t e0 = f.pos; e0 < table_len; e0 += 64) {
                const int64_t e = e0 + lane;
                const int64_t v = e < table_len ? sems[e] : 0;
                const uint64_t m = __ballot(v != 0);
                if (m) { nx = (int64_t)readlane64((uint64_t)v, __ffsll((unsigned long long)m) - 1); break; }
            }
            const int64_t end = nx ? nx - 1 : capacity;
            if (sp < 1 || sp > capacity || end < sp || end > capacity) r.err = 2u;      // tables out of step with the slots
            else { r.lo = sp; r.hi = end; }
        }
    }
    return r;
}

// The end of an emit kernel (256 threads, every one arrives): the error bits of the workgroup go into the scratch word, and the
// workgroup that takes the last ticket hands {error word, seq} to pinned memory.
__device__ __forceinline__ void emit_epilogue(uint32_t err, int lane, int wv, uint32_t* err_word, uint32_t* ticket,
                                              unsigned long long* pinned, unsigned long long seq) {
    __shared__ uint32_t sErr[4];
    err = wave_or(err);
    if (lane == 0) sErr[wv] = err;
    __syncthreads();
    if (threadIdx.x != 0) return;
    err = sErr[0] | sErr[1] | sErr[2] | sErr[3];
    if (err) __hip_atomic_fetch_or(err_word, err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_s_waitcnt(0);
    const uint32_t tk = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tk != gridDim.x - 1) return;
    // the last workgroup: every other one has added its bits before taking its ticket
    const uint32_t e = __hip_atomic_load(err_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(pinned + 0, (unsigned long long)e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    publish_seq(pinned + 1, seq);
}

}  // namespace dsa
