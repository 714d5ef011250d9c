// csrc/combine.hip — K-combine: the stored cells of a colmajor orientation as (I, J, V) triples in slot order (the findnz order), the
// row key shifted by row_off, the key of the owning partition by col_off, the value multiplied by `scale` — what the device builder
// (build.hip) takes.  dsa_mat_combine runs it once per operand into one pooled buffer and builds the result from the concatenation;
// the kernel adds nothing, a key present in both operands is summed by the builder like any duplicate.
//
// The shape of compress.hip, whose tile count it shares (export_dev.h: k_cx_count): with O(s) = occupied slots in front of s and
// R(s) = semaphores at or in front of s the cell at s goes to position O(s) - R(s).  Three launches, no host wait in between:
//   k_cx_count  one wave per 2048-slot tile: occupied slots; the table: live semaphores per tile and the id of the last one
//   k_cb_scan   one workgroup: exclusive prefixes of both counts, the totals checked against the host's counts; the ids scanned with
//               a max: carry[t] = the last semaphore in front of tile t
//   k_cb_emit   one wave per tile: keys and values streamed once (non-temporal), all words of a group requested up front.  The owner
//               of a cell is the last semaphore at or in front of it: inside the tile its value is the id (col_keys[id - 1]), in front
//               of the tile's first semaphore it is the carry — no wave walks back through the slot array.  Per wave one 64-bit
//               atomicMax for each end of the two key ranges; the last workgroup hands error word and ranges to pinned memory.
// The slot arrays, the tables and both epochs stay untouched.  Bytes: (kb + 8) * capacity + capacity / 8 (+ the bitmap once more in
// k_cx_count) + 16 * table_len in, 24 * nnz out.
#include "combine.h"
#include "export_dev.h"
#include <climits>
#include <type_traits>

namespace dsa {

// scratch: the tile arrays of k_cx_count, the four range words, the last-semaphore ids (one memset covers sem_cnt .. last_id)
struct CbScratch {
    CxScratch cx;
    unsigned long long* acc;            // {row min, row max, column min, column max} in the form of cb_range (combine.h)
    unsigned long long* last_id;        // per tile: k_cx_count the id of its last semaphore (0: none), k_cb_scan the carry into it
};
static CbScratch cb_carve(void* base, int64_t tiles) {
    CbScratch s;
    s.cx = cx_carve(base, tiles);
    s.acc = reinterpret_cast<unsigned long long*>(static_cast<char*>(base) + cx_scratch_bytes(tiles));
    s.last_id = s.acc + 4;
    return s;
}
size_t combine_scratch_bytes(int64_t capacity) { return cx_scratch_bytes(cx_tiles(capacity)) + 32 + (size_t)cx_tiles(capacity) * 8; }

// One workgroup of EX_SCAN_THREADS: a[i] = max of a[0..i) (0 for i = 0), one entry per thread and step, the max of the steps in front
// carried along (16 steps for the 2^25 slots of a 10^7-entry matrix: nothing beside the emit).
__device__ __forceinline__ void block_excl_max(unsigned long long* a, int64_t n) {
    __shared__ unsigned long long sM[EX_SCAN_THREADS];
    const int t = threadIdx.x;
    unsigned long long carry = 0;
    for (int64_t c0 = 0; c0 < n; c0 += EX_SCAN_THREADS) {
        const int64_t i = c0 + t;
        sM[t] = i < n ? a[i] : 0ull;
        __syncthreads();
        for (int o = 1; o < EX_SCAN_THREADS; o <<= 1) {          // inclusive scan (Hillis-Steele)
            const unsigned long long x = t >= o ? sM[t - o] : 0ull;
            __syncthreads();
            if (x > sM[t]) sM[t] = x;
            __syncthreads();
        }
        const unsigned long long in_front = t > 0 ? sM[t - 1] : 0ull, top = sM[EX_SCAN_THREADS - 1];
        if (i < n) a[i] = in_front > carry ? in_front : carry;
        if (top > carry) carry = top;
        __syncthreads();
    }
}

__global__ __launch_bounds__(EX_SCAN_THREADS) void k_cb_scan(CbScratch s, int64_t nparts, int64_t nnz) {
    unsigned long long carry_o, carry_s;
    block_excl_scan2(s.cx.occ_cnt, s.cx.sem_cnt, s.cx.tiles,
                     [&](int64_t i, unsigned long long ro, unsigned long long rs) { s.cx.occ_off[i] = (int64_t)ro; s.cx.sem_off[i] = (int64_t)rs; },
                     carry_o, carry_s);
    if (threadIdx.x == 0 && ((int64_t)carry_s != nparts || (int64_t)(carry_o - carry_s) != nnz)) atomicOr(s.cx.err, CB_ASSERT);
    block_excl_max(s.last_id, s.cx.tiles);
}

struct CbArgs {
    int64_t* I; int64_t* J; double* V;
    int64_t nnz, row_off, col_off;
    double scale;
    unsigned long long* pinned;         // CB_WORDS words
    unsigned long long seq;
};

__device__ __forceinline__ int64_t wave_min_i64(int64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int64_t y = __shfl_xor(v, o, 64); v = y < v ? y : v; }
    return v;
}
__device__ __forceinline__ int64_t wave_max_i64(int64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int64_t y = __shfl_xor(v, o, 64); v = y > v ? y : v; }
    return v;
}
__device__ __forceinline__ int64_t shifted(int64_t key, int64_t off) { return (int64_t)((uint64_t)key + (uint64_t)off); }      // (wraps: the host refuses a range that leaves int64)

// one wave per tile
template <bool WIDE>
__global__ __launch_bounds__(256) void k_cb_emit(KeyArr keys, const double* __restrict__ vals, const uint64_t* __restrict__ occ,
                                                 int64_t capacity, const int64_t* __restrict__ col_keys, int64_t table_len, CbScratch s,
                                                 CbArgs a) {
    typedef typename std::conditional<WIDE, int64_t, int32_t>::type key_t;
    const key_t* __restrict__ kp = static_cast<const key_t*>(keys.p);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t t = (int64_t)blockIdx.x * 4 + wv;
    const uint64_t below = mask_lt(lane);
    uint32_t err = 0;
    int64_t rlo = INT64_MAX, rhi = INT64_MIN, clo = INT64_MAX, chi = INT64_MIN;
    if (t < s.cx.tiles) {
        const int64_t w0 = t * EX_WORDS, nwords = (capacity + 63) >> 6;
        const uint64_t myword = lane < EX_WORDS && w0 + lane < nwords ? __builtin_nontemporal_load(occ + w0 + lane) : 0ull;
        int64_t run_o = s.cx.occ_off[t], run_r = s.cx.sem_off[t];
        // the owner of the cells in front of the tile's first semaphore: the carry (0: no semaphore in front of this tile)
        const int64_t carry = (int64_t)s.last_id[t];
        bool have_run = carry >= 1 && carry <= table_len;
        int64_t c_run = have_run ? col_keys[carry - 1] : 0;
        if (carry < 0 || carry > table_len) err |= CB_ASSERT;
        for (int q = 0; q < EX_WORDS; q += EX_U) {
            uint64_t wd[EX_U];
            int64_t k[EX_U], ck[EX_U];
            double v[EX_U];
#pragma unroll
            for (int u = 0; u < EX_U; ++u) {
                wd[u] = readlane64(myword, q + u);
                const int64_t i = ((w0 + q + u) << 6) + lane;
                k[u] = -1; v[u] = 0.0;
                if ((wd[u] >> lane) & 1ull) { k[u] = (int64_t)__builtin_nontemporal_load(kp + i); v[u] = __builtin_nontemporal_load(vals + i); }
            }
#pragma unroll
            for (int u = 0; u < EX_U; ++u) {        // keys of the partitions whose semaphores these words hold (semaphore value = id)
                ck[u] = 0;
                if (k[u] == SEM_KEY && ((wd[u] >> lane) & 1ull)) {
                    const int64_t p = (int64_t)v[u];
                    if (p >= 1 && p <= table_len) ck[u] = col_keys[p - 1]; else err |= CB_ASSERT;
                }
            }
#pragma unroll
            for (int u = 0; u < EX_U; ++u) {
                const bool bit = (wd[u] >> lane) & 1ull;
                const bool sem = bit && k[u] == SEM_KEY;
                const uint64_t sb = __ballot(sem);
                const uint64_t pm = sb & below;                                   // semaphores of this word in front of this lane
                const int64_t c_sh = __shfl(ck[u], pm ? 63 - __clzll((unsigned long long)pm) : 0, 64);
                if (bit && !sem) {
                    const int64_t pos = run_o + popc64(wd[u] & below) - (run_r + popc64(pm));
                    if ((pm || have_run) && pos >= 0 && pos < a.nnz) {
                        const int64_t c = pm ? c_sh : c_run;
                        const int64_t i2 = shifted(k[u], a.row_off), j2 = shifted(c, a.col_off);
                        __builtin_nontemporal_store(i2, a.I + pos);
                        __builtin_nontemporal_store(j2, a.J + pos);
                        __builtin_nontemporal_store(a.scale * v[u], a.V + pos);
                        if (i2 == 0 || j2 == 0) err |= CB_ZERO_KEY;
                        rlo = k[u] < rlo ? k[u] : rlo; rhi = k[u] > rhi ? k[u] : rhi;
                        clo = c < clo ? c : clo; chi = c > chi ? c : chi;
                    } else {
                        err |= CB_ASSERT;                                         // a cell without a partition, or more cells than counted
                    }
                }
                if (sb) { c_run = __shfl(ck[u], 63 - __clzll((unsigned long long)sb), 64); have_run = true; }
                run_o += popc64(wd[u]);
                run_r += popc64(sb);
            }
        }
    }
    // the ranges of the wave: one atomic per end, complete in L2 before the workgroup's ticket (emit_last)
    rlo = wave_min_i64(rlo); rhi = wave_max_i64(rhi); clo = wave_min_i64(clo); chi = wave_max_i64(chi);
    if (lane == 0 && rhi >= rlo) {
        constexpr unsigned long long SIGN = 0x8000000000000000ull;
        atomicMax(s.acc + 0, ~((unsigned long long)rlo ^ SIGN));
        atomicMax(s.acc + 1, (unsigned long long)rhi ^ SIGN);
        atomicMax(s.acc + 2, ~((unsigned long long)clo ^ SIGN));
        atomicMax(s.acc + 3, (unsigned long long)chi ^ SIGN);
        __builtin_amdgcn_s_waitcnt(0);
    }
    if (!emit_last(err, lane, wv, s.cx.err, s.cx.ticket)) return;
    const uint32_t e = __hip_atomic_load(s.cx.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(a.pinned + 0, (unsigned long long)e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
#pragma unroll
    for (int w = 0; w < 4; ++w)
        __hip_atomic_store(a.pinned + 1 + w, __hip_atomic_load(s.acc + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
    publish_seq(a.pinned + CB_WORDS - 1, a.seq);
}

hipError_t launch_combine(const SlotView& V, int64_t nparts, int64_t nnz, int64_t* d_I, int64_t* d_J, double* d_V, double scale,
                          int64_t row_off, int64_t col_off, void* scratch, unsigned long long* pinned, unsigned long long seq,
                          hipStream_t stream) {
    if (V.capacity < 0 || V.table_len < 0 || nnz < 0 || V.sems == nullptr || V.part_keys == nullptr) return hipErrorInvalidValue;
    if (nnz > 0 && (!d_I || !d_J || !d_V)) return hipErrorInvalidValue;
    const int64_t tiles = cx_tiles(V.capacity);
    const CbScratch s = cb_carve(scratch, tiles);
    // sem_cnt .. ticket, the range words, the last-semaphore ids: contiguous
    hipError_t e = hipMemsetAsync(s.cx.sem_cnt, 0, (size_t)tiles * sizeof(uint32_t) + 8 + 32 + (size_t)tiles * 8, stream);
    if (e != hipSuccess) return e;
    const int64_t tile_blocks = (tiles + 3) / 4, table_blocks = (V.table_len + 255) / 256;
    hipLaunchKernelGGL(k_cx_count<true>, dim3((unsigned)(tile_blocks + table_blocks)), dim3(256), 0, stream, V.occ, V.capacity, V.sems, V.part_live,
                       V.table_len, tile_blocks, s.cx, s.last_id);
    hipLaunchKernelGGL(k_cb_scan, dim3(1), dim3(EX_SCAN_THREADS), 0, stream, s, nparts, nnz);
    const CbArgs a{d_I, d_J, d_V, nnz, row_off, col_off, scale, pinned, seq};
    if (V.keys.wide)
        hipLaunchKernelGGL(k_cb_emit<true>, dim3((unsigned)tile_blocks), dim3(256), 0, stream, V.keys, V.vals, V.occ, V.capacity, V.part_keys,
                           V.table_len, s, a);
    else
        hipLaunchKernelGGL(k_cb_emit<false>, dim3((unsigned)tile_blocks), dim3(256), 0, stream, V.keys, V.vals, V.occ, V.capacity, V.part_keys,
                           V.table_len, s, a);
    return hipGetLastError();
}

}  // namespace dsa
