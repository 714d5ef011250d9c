// csrc/compress.hip — K-compress: the stored entries of one orientation in compressed form (CSC from colmajor, CSR from rowmajor).
//
// A cell at slot s belongs to the partition of the last semaphore in front of it, and the k-th semaphore in slot order is the k-th
// live partition (the tables are in key order at every API boundary).  With O(s) = occupied slots in front of s and R(s) = semaphores
// at or in front of s, the cell goes to position O(s) - R(s) of idx / val, and the partition whose semaphore sits at s starts at
// O(s) - R(s) + 1.  Three launches, no host wait in between:
//   k_cx_count  (export_dev.h) one wave per 2048-slot tile: occupied slots (a popcount of the tile's 32 bitmap words); the table: live semaphores per tile
//   k_cx_scan   one workgroup: exclusive prefixes of both counts, the totals checked against the host's counts, ptr behind the last
//               live partition
//   k_cx_emit   one wave per tile: keys and values streamed once (non-temporal), cells to idx / val, and at every semaphore the ptr run
//               from the previous live key up to its own (as zero_fill_front does for the rows of y); the last workgroup hands the
//               error word to pinned memory
// The slot arrays, the tables and both epochs stay untouched.  Bytes: (kb + 8) * capacity + capacity / 8 (+ the bitmap once more in
// k_cx_count) + 17 * table_len in, (ib + 8) * nnz + ib * (dim + 1) out.
#include "compress.h"
#include "export_dev.h"
#include <climits>
#include <type_traits>

namespace dsa {

size_t compress_scratch_bytes(int64_t capacity) { return cx_scratch_bytes(cx_tiles(capacity)); }

// one workgroup: occ_off / sem_off; totals against the host's counts; ptr[k] = base + nnz for k from the last live key to dim_out
template <typename IT>
__global__ __launch_bounds__(EX_SCAN_THREADS) void k_cx_scan(CxScratch s, const int64_t* __restrict__ sems, const int64_t* __restrict__ col_keys,
                                                             int64_t table_len, int64_t nparts, int64_t nnz, int64_t dim_out, int64_t base,
                                                             IT* __restrict__ ptr) {
    __shared__ long long sLast;
    const int t = threadIdx.x;
    unsigned long long carry_o, carry_s;
    block_excl_scan2(s.occ_cnt, s.sem_cnt, s.tiles,
                     [&](int64_t i, unsigned long long ro, unsigned long long rs) { s.occ_off[i] = (int64_t)ro; s.sem_off[i] = (int64_t)rs; },
                     carry_o, carry_s);
    // the last live partition (tombstones at the end of the tables are skipped, 1024 entries per step)
    if (t == 0) sLast = -1;
    __syncthreads();
    for (int64_t hi = table_len - 1; hi >= 0; hi -= EX_SCAN_THREADS) {
        const int64_t i = hi - t;
        if (i >= 0 && sems[i] != 0) atomicMax(&sLast, (long long)i);
        __syncthreads();
        const bool found = sLast >= 0;
        __syncthreads();
        if (found) break;
    }
    const int64_t c_last = sLast >= 0 ? col_keys[sLast] : INT64_MIN;
    if (t == 0) {
        uint32_t e = 0;
        if ((int64_t)carry_s != nparts || (int64_t)(carry_o - carry_s) != nnz) e |= 2u;
        if (c_last <= 0 && nnz > 0) e |= 1u;                    // every stored entry lies in a partition whose key is below 1
        if (e) atomicOr(s.err, e);
    }
    const IT v = (IT)(base + nnz);
    for (int64_t k = (c_last > 0 ? c_last : 0) + t; k <= dim_out; k += EX_SCAN_THREADS) __builtin_nontemporal_store(v, ptr + k);
}

struct CxArgs {
    void* ptr; void* idx; double* val;
    int64_t dim_out, dim_in, nnz, base;
    unsigned long long* pinned;         // {error word, sequence number}
    unsigned long long seq;
};

// one wave per tile.  Error bits: 1 a stored entry outside size(m), 2 slots and tables disagree.
template <bool WIDE, typename IT>
__global__ __launch_bounds__(256) void k_cx_emit(KeyArr keys, const double* __restrict__ vals, const uint64_t* __restrict__ occ,
                                                 int64_t capacity, const int64_t* __restrict__ sems, const int64_t* __restrict__ col_keys,
                                                 int64_t table_len, CxScratch s, CxArgs a) {
    typedef typename std::conditional<WIDE, int64_t, int32_t>::type key_t;
    const key_t* __restrict__ kp = static_cast<const key_t*>(keys.p);
    IT* __restrict__ ptr = static_cast<IT*>(a.ptr);
    IT* __restrict__ idx = static_cast<IT*>(a.idx);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t t = (int64_t)blockIdx.x * 4 + wv;
    const uint64_t below = mask_lt(lane);
    uint32_t err = 0;
    if (t < s.tiles) {
        const int64_t w0 = t * EX_WORDS, nwords = (capacity + 63) >> 6;
        const uint64_t myword = lane < EX_WORDS && w0 + lane < nwords ? __builtin_nontemporal_load(occ + w0 + lane) : 0ull;
        int64_t run_o = s.occ_off[t], run_r = s.sem_off[t];
        int64_t c_run = 0;
        bool have_prev = false;          // c_run holds the key of the last semaphore seen in this tile
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
                if (k[u] == SEM_KEY) {
                    const int64_t p = (int64_t)v[u];
                    if (p >= 1 && p <= table_len) ck[u] = col_keys[p - 1]; else err |= 2u;
                }
            }
#pragma unroll
            for (int u = 0; u < EX_U; ++u) {
                const bool bit = (wd[u] >> lane) & 1ull;
                const bool sem = bit && k[u] == SEM_KEY;
                const uint64_t sb = __ballot(sem);
                const int64_t o = run_o + popc64(wd[u] & below);                  // occupied slots in front of this one
                const int64_t r = run_r + popc64(sb & below) + (sem ? 1 : 0);     // semaphores up to this one
                if (bit && !sem) {
                    const int64_t pos = o - r;
                    if (pos >= 0 && pos < a.nnz) {
                        __builtin_nontemporal_store((IT)(k[u] - 1 + a.base), idx + pos);
                        __builtin_nontemporal_store(v[u], a.val + pos);
                    } else {
                        err |= 2u;
                    }
                    if (k[u] < 1 || k[u] > a.dim_in) err |= 1u;
                }
                if (sb) {
                    // key of the previous live partition: the semaphore in front in this word, the last one of an earlier word of this
                    // tile, or (first semaphore of the tile) the table, skipping tombstones
                    const uint64_t pm = sb & below;
                    const int src = pm ? 63 - __clzll(pm) : 0;
                    const int64_t c_sh = __shfl(ck[u], src, 64);
                    if (sem) {
                        int64_t c_prev;
                        if (pm) c_prev = c_sh;
                        else if (have_prev) c_prev = c_run;
                        else {
                            int64_t j = (int64_t)v[u] - 2;
                            while (j >= 0 && sems[j] == 0) --j;
                            c_prev = j >= 0 ? col_keys[j] : INT64_MIN;
                        }
                        const int64_t st = o - r + 1;                 // cells of the partitions in front of this one
                        const int64_t c = ck[u];
                        if (c_prev <= 0 && c >= 1 && st != 0) err |= 1u;                          // cells in partitions keyed below 1
                        if (c_prev <= a.dim_out && c > a.dim_out && st != a.nnz) err |= 1u;     // ... or above dim_out
                        const int64_t lo = c_prev > 0 ? c_prev : 0, hi = c - 1 < a.dim_out ? c - 1 : a.dim_out;
                        const IT pv = (IT)(a.base + st);
                        for (int64_t kk = lo; kk <= hi; ++kk) __builtin_nontemporal_store(pv, ptr + kk);
                    }
                    c_run = __shfl(ck[u], 63 - __clzll(sb), 64);
                    have_prev = true;
                }
                run_o += popc64(wd[u]);
                run_r += popc64(sb);
            }
        }
    }
    emit_epilogue(err, lane, wv, s.err, s.ticket, a.pinned, a.seq);
}

template <bool WIDE, typename IT>
static void launch_emit_t(unsigned grid, hipStream_t stream, const SlotView& V, const CxScratch& s, const CxArgs& a) {
    hipLaunchKernelGGL((k_cx_emit<WIDE, IT>), dim3(grid), dim3(256), 0, stream, V.keys, V.vals, V.occ, V.capacity, V.sems, V.part_keys, V.table_len,
                       s, a);
}

hipError_t launch_to_compressed(const SlotView& V, int64_t nparts, int64_t nnz, int64_t dim_out, int64_t dim_in, int32_t index_bits, int64_t base,
                                void* d_ptr, void* d_idx, double* d_vals, void* scratch, unsigned long long* out2_pinned,
                                unsigned long long seq, hipStream_t stream) {
    if (V.capacity < 0 || V.table_len < 0 || dim_out < 0 || (index_bits != 32 && index_bits != 64)) return hipErrorInvalidValue;
    const int64_t tiles = cx_tiles(V.capacity);
    const CxScratch s = cx_carve(scratch, tiles);
    hipError_t e = hipMemsetAsync(s.sem_cnt, 0, (size_t)tiles * sizeof(uint32_t) + 8, stream);
    if (e != hipSuccess) return e;
    const int64_t tile_blocks = (tiles + 3) / 4, table_blocks = (V.table_len + 255) / 256;
    hipLaunchKernelGGL(k_cx_count<false>, dim3((unsigned)(tile_blocks + table_blocks)), dim3(256), 0, stream, V.occ, V.capacity, V.sems, V.part_live,
                       V.table_len, tile_blocks, s, static_cast<unsigned long long*>(nullptr));
    if (index_bits == 32)
        hipLaunchKernelGGL(k_cx_scan<int32_t>, dim3(1), dim3(EX_SCAN_THREADS), 0, stream, s, V.sems, V.part_keys, V.table_len, nparts, nnz,
                           dim_out, base, static_cast<int32_t*>(d_ptr));
    else
        hipLaunchKernelGGL(k_cx_scan<int64_t>, dim3(1), dim3(EX_SCAN_THREADS), 0, stream, s, V.sems, V.part_keys, V.table_len, nparts, nnz,
                           dim_out, base, static_cast<int64_t*>(d_ptr));
    CxArgs a{d_ptr, d_idx, d_vals, dim_out, dim_in, nnz, base, out2_pinned, seq};
    const unsigned grid = (unsigned)tile_blocks;
    if (V.keys.wide) {
        if (index_bits == 32) launch_emit_t<true, int32_t>(grid, stream, V, s, a);
        else launch_emit_t<true, int64_t>(grid, stream, V, s, a);
    } else {
        if (index_bits == 32) launch_emit_t<false, int32_t>(grid, stream, V, s, a);
        else launch_emit_t<false, int64_t>(grid, stream, V, s, a);
    }
    return hipGetLastError();
}

}  // namespace dsa
