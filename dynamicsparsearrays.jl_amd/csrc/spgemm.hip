// csrc/spgemm.hip — the batched sparse-x product: Y = A S (colmajor walked) / Y = A' S (rowmajor) for k sparse columns of S, both
// operands and the result CSC in HBM.  Column j of Y is what the reference's _mul (src/operations.jl:62-135) gives for column j of
// S: the touched rows only, ascending, a value summed from +0.0 over the stored entries of the column in their order, each matching
// partition in slot order, one multiply then one add per term.  No float atomics: the bits of a value do not depend on timing.
//
// A two-phase (count, then emit) row-wise Gustavson product in three groups of launches with a host wait behind each:
//   k_spg_bound     one wave per stored entry of S: its column (search over xptr), the input contract (xidx strictly ascending within
//                   a column; xptr checked by one thread per column), the span of the partition its key names (find_dev.h:
//                   key_span, the lookup of the selected export), the popcount of the span; (lo, hi, cells) per entry go to scratch so
//                   that no later pass locates again, ub[c] += cells (integer atomics)
//   k_spg_classify  one workgroup: the columns with ub > SPG_SMALL_MAX go on the list of the long ones; {error, long columns} handed over
//   (host: the input contract, the slabs the long columns need — DSA_EARG when a single one exceeds SPG_SLAB_BYTES_MAX)
//   k_spg_lds<0>    one wave per column with 0 < ub <= SPG_SMALL_MAX: the entries in order, each span 64 slots at a time; a lane with a
//                   cell claims or finds its row in an open-addressing table in LDS (atomicCAS on the key word, linear probing bounded
//                   by SPG_TABLE_SLOTS); count = claimed entries
//   k_spg_slab<0>   one workgroup per slab, looping over the long columns: bits of the touched rows set with atomicOr, counted and
//                   cleared again
//   k_spg_scan      counts -> yptr and the offsets of the emit; {error, total} handed over
//   (host: cap and the 32-bit rule)
//   k_spg_lds<1>    the same walk with a plain read-add-write of the sum beside the key (keys within a partition are distinct, so no
//                   two lanes of a step share a row; the steps of the one wave are ordered: that is the summation order), then the
//                   claimed entries packed to the front of the table, sorted by key (bitonic, in LDS) and written at yptr[c]
//   k_spg_slab<1>   the entries in order, plain adds on distinct rows with a workgroup barrier between two entries, then the bitmap
//                   walked in ascending order: (row, sum) out, sum and bits zero again — a slab is all zero between two columns
//   k_spg_done      the error word handed over
// No loop depends on the table being non-full; an emit never writes outside the range its count reserved.
#include "spgemm.h"
#include "export_dev.h"

namespace dsa {

constexpr int SPG_TABLE_BITS = 11;
static_assert((int64_t(1) << SPG_TABLE_BITS) == SPG_TABLE_SLOTS, "SPG_TABLE_SLOTS is a power of two");
static_assert(SPG_TABLE_SLOTS >= 2 * SPG_SMALL_MAX, "the LDS table is at most half full");
constexpr int64_t SPG_GRID_MAX = int64_t(1) << 20;      // workgroups per launch: beyond it they stride

struct SpgScratch {
    uint32_t* err; uint32_t* n_large;                    // zeroed with ub by the one memset
    unsigned long long* ub;                              // [k] stored cells column c will visit
    int64_t* colbeg;                                     // [k + 1] first entry of column c (xptr - base)
    int64_t* cnt;                                        // [k + 1] touched rows of column c (count), then their exclusive prefix (scan)
    int64_t* lo; int64_t* hi; int64_t* cells;            // [nnzx] span [lo, hi) (0-based slots) and cells of entry e
    int32_t* large;                                      // [k] the long columns, in any order
};
static SpgScratch spg_carve(void* base, int64_t k, int64_t nnzx) {
    SpgScratch s;
    char* p = static_cast<char*>(base);
    s.err = reinterpret_cast<uint32_t*>(p);
    s.n_large = s.err + 1;
    s.ub = reinterpret_cast<unsigned long long*>(p + 16);
    s.colbeg = reinterpret_cast<int64_t*>(s.ub + k);
    s.cnt = s.colbeg + k + 1;
    s.lo = s.cnt + k + 1;
    s.hi = s.lo + nnzx;
    s.cells = s.hi + nnzx;
    s.large = reinterpret_cast<int32_t*>(s.cells + nnzx);
    return s;
}
size_t spgemm_scratch_bytes(int64_t k, int64_t nnzx) { return 16 + (size_t)k * 8 + (size_t)(k + 1) * 16 + (size_t)nnzx * 24 + (size_t)k * 4 + 8; }
int64_t spgemm_slab_words(int64_t ny) { const int64_t nwords = (ny + 63) >> 6; return nwords * 64 + nwords; }

__device__ __forceinline__ int64_t spg_ld(const void* p, int64_t i, int bits32) {
    return bits32 ? (int64_t)static_cast<const int32_t*>(p)[i] : static_cast<const int64_t*>(p)[i];
}

// ---- phase 1 --------------------------------------------------------------------------------------------------------------------
// virtual workgroups [0, eblocks): four entries each, one wave per entry; [eblocks, eblocks + cblocks): 256 column boundaries each
__global__ __launch_bounds__(256) void k_spg_bound(SlotView V, SpgIndex ix, const void* __restrict__ xptr,
                                                   const void* __restrict__ xidx, int64_t k, int64_t nnzx, SpgScratch s, int64_t eblocks,
                                                   int64_t cblocks) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int64_t vb = blockIdx.x; vb < eblocks + cblocks; vb += gridDim.x) {
        if (vb >= eblocks) {
            const int64_t j = (vb - eblocks) * 256 + threadIdx.x;
            if (j > k) continue;
            const int64_t p = spg_ld(xptr, j, ix.bits32) - ix.base;
            bool bad = p < 0 || p > nnzx || (j == 0 && p != 0) || (j == k && p != nnzx);
            if (j < k) bad = bad || spg_ld(xptr, j + 1, ix.bits32) - ix.base < p;
            s.colbeg[j] = p < 0 ? 0 : (p > nnzx ? nnzx : p);
            if (bad) atomicOr(s.err, SPG_ERR_INPUT);
            continue;
        }
        const int64_t e = vb * 4 + wv;
        if (e >= nnzx) continue;
        // the column of entry e: the last c with xptr[c] - base <= e (a search over garbage stays inside [0, k]; the column
        // threads report what is wrong with xptr)
        int64_t L = 0, H = k + 1;
        while (L < H) {
            const int64_t mid = (L + H) >> 1;
            if (spg_ld(xptr, mid, ix.bits32) - ix.base <= e) L = mid + 1; else H = mid;
        }
        const int64_t c = L - 1;
        uint32_t err = 0;
        int64_t lo = 0, hi = 0, cells = 0;
        if (c < 0 || c >= k) {
            err = SPG_ERR_INPUT;
        } else {
            const int64_t key = spg_ld(xidx, e, ix.bits32) + 1 - ix.base;
            if (e > 0 && e > spg_ld(xptr, c, ix.bits32) - ix.base && spg_ld(xidx, e - 1, ix.bits32) + 1 - ix.base >= key) err = SPG_ERR_INPUT;
            // a key without a live partition (never written, deleted, beyond the table, below 1) contributes nothing
            const KeySpan sp = key_span(V, key, INT64_MAX, lane);
            if (sp.err & 2u) err |= SPG_ERR_STEP;
            lo = sp.lo; hi = sp.hi;
            cells = hi > lo ? sel_span_popc(V.occ, lo, hi, lane) : 0;
        }
        if (lane != 0) continue;
        s.lo[e] = lo; s.hi[e] = hi; s.cells[e] = cells;
        if (cells > 0) atomicAdd(s.ub + c, (unsigned long long)cells);
        if (err) atomicOr(s.err, err);
    }
}

__global__ __launch_bounds__(1024) void k_spg_classify(SpgScratch s, int64_t k, unsigned long long* pinned, unsigned long long seq) {
    for (int64_t c = threadIdx.x; c < k; c += 1024)
        if (s.ub[c] > (unsigned long long)SPG_SMALL_MAX) s.large[atomicAdd(s.n_large, 1u)] = (int32_t)c;
    __syncthreads();
    if (threadIdx.x != 0) return;
    const uint32_t e = __hip_atomic_load(s.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t nl = __hip_atomic_load(s.n_large, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(pinned + 0, (unsigned long long)e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(pinned + 1, (unsigned long long)nl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    publish_seq(pinned + 2, seq);
}

// ---- the LDS path: one wave (= one workgroup) per column -----------------------------------------------------------------------------
__device__ __forceinline__ void spg_store_idx(void* yidx, int64_t pos, int64_t row, SpgIndex ix) {
    if (ix.bits32) static_cast<int32_t*>(yidx)[pos] = (int32_t)(row - 1 + ix.base);
    else static_cast<int64_t*>(yidx)[pos] = row - 1 + ix.base;
}

template <bool EMIT>
__global__ __launch_bounds__(64) void k_spg_lds(KeyArr keys, const double* __restrict__ vals, const uint64_t* __restrict__ occ, SpgScratch s,
                                                const double* __restrict__ xval, int64_t k, int64_t ny, SpgIndex ix, void* yidx,
                                                double* __restrict__ yval) {
    constexpr int SLOTS = (int)SPG_TABLE_SLOTS;
    __shared__ unsigned long long tkey[SLOTS];           // 0: free (row keys start at 1)
    __shared__ double tval[EMIT ? SLOTS : 1];
    const int lane = threadIdx.x;
    uint32_t err = 0;
    for (int64_t c = blockIdx.x; c < k; c += gridDim.x) {
        const unsigned long long ub = s.ub[c];
        if (ub > (unsigned long long)SPG_SMALL_MAX) continue;          // the slab path's
        if (ub == 0) { if (!EMIT && lane == 0) s.cnt[c] = 0; continue; }
        const int64_t off = EMIT ? s.cnt[c] : 0, expect = EMIT ? s.cnt[c + 1] - off : 0;
        for (int i = lane; i < SLOTS; i += 64) { tkey[i] = 0ull; if (EMIT) tval[i] = 0.0; }
        __syncthreads();
        uint32_t claimed = 0;
        const int64_t e1 = s.colbeg[c + 1];
        for (int64_t e = s.colbeg[c]; e < e1; ++e) {
            if (s.cells[e] == 0) continue;
            const int64_t lo = s.lo[e], hi = s.hi[e];
            const double xv = EMIT ? xval[e] : 0.0;
            for (int64_t w = lo >> 6; w <= (hi - 1) >> 6; ++w) {
                const uint64_t word = occ[w] & word_range_mask(w, lo, hi - 1);
                if (word == 0ull) continue;                            // (wave-uniform)
                if ((word >> lane) & 1ull) {
                    const int64_t i = (w << 6) + lane;
                    const int64_t row = keys[i];
                    if (row == SEM_KEY) err |= SPG_ERR_STEP;
                    else if (row < 1 || row > ny) err |= SPG_ERR_BOUNDS;
                    else {
                        uint32_t h = (uint32_t)(((unsigned long long)row * 0x9E3779B97F4A7C15ull) >> (64 - SPG_TABLE_BITS));
                        bool found = false;
                        for (int p = 0; p < SLOTS; ++p) {              // bounded whatever the table holds
                            const unsigned long long prev = atomicCAS(&tkey[h], 0ull, (unsigned long long)row);
                            if (prev == 0ull) { ++claimed; found = true; break; }
                            if (prev == (unsigned long long)row) { found = true; break; }
                            h = (h + 1) & (SLOTS - 1);
                        }
                        if (!found) err |= SPG_ERR_PROBE;
                        else if (EMIT) tval[h] = tval[h] + xv * vals[i];
                    }
                }
                __syncthreads();                                       // one wave: the next step sees this step's table
            }
        }
        const uint32_t n = wave_reduce_add(claimed);
        if (!EMIT) {
            if (lane == 0) s.cnt[c] = (int64_t)n;
            __syncthreads();
            continue;
        }
        if ((int64_t)n != expect || n > (uint32_t)SPG_SMALL_MAX) { err |= SPG_ERR_STEP; __syncthreads(); continue; }
        // pack the claimed entries to the front: a block is read before anything at or in front of it is overwritten
        int run = 0;
        for (int b = 0; b < SLOTS; b += 64) {
            const unsigned long long kk = tkey[b + lane];
            const double vv = tval[b + lane];
            const uint64_t m = __ballot(kk != 0ull);
            __syncthreads();
            if (kk != 0ull) { const int pos = run + popc64(m & mask_lt(lane)); tkey[pos] = kk; tval[pos] = vv; }
            run += popc64(m);
            __syncthreads();
        }
        int P = 64;
        while (P < (int)n) P <<= 1;
        for (int i = (int)n + lane; i < P; i += 64) tkey[i] = ~0ull;
        __syncthreads();
        for (int size = 2; size <= P; size <<= 1) {
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                for (int t = lane; t < (P >> 1); t += 64) {
                    const int i = ((t / stride) * 2 * stride) + (t % stride), j = i + stride;
                    const bool up = (i & size) == 0;
                    const unsigned long long a = tkey[i], b = tkey[j];
                    if ((a > b) == up) {
                        const double va = tval[i], vb = tval[j];
                        tkey[i] = b; tkey[j] = a; tval[i] = vb; tval[j] = va;
                    }
                }
                __syncthreads();
            }
        }
        for (int i = lane; i < (int)n; i += 64) {
            spg_store_idx(yidx, off + i, (int64_t)tkey[i], ix);
            yval[off + i] = tval[i];
        }
        __syncthreads();
    }
    err = wave_or(err);
    if (lane == 0 && err) atomicOr(s.err, err);
}

// ---- the slab path: one workgroup per slab, looping over the long columns ---------------------------------------------------------------
template <bool EMIT>
__global__ __launch_bounds__(256) void k_spg_slab(KeyArr keys, const double* __restrict__ vals, const uint64_t* __restrict__ occ, SpgScratch s,
                                                  const double* __restrict__ xval, int64_t ny, unsigned long long* slabs, int64_t slab_words,
                                                  SpgIndex ix, void* yidx, double* __restrict__ yval) {
    __shared__ unsigned long long sSum[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t nwords = (ny + 63) >> 6;
    double* acc = reinterpret_cast<double*>(slabs + (int64_t)blockIdx.x * slab_words);
    unsigned long long* bm = slabs + (int64_t)blockIdx.x * slab_words + nwords * 64;
    const int64_t nl = (int64_t)*s.n_large;
    uint32_t err = 0;
    for (int64_t li = blockIdx.x; li < nl; li += gridDim.x) {
        const int64_t c = s.large[li];
        const int64_t e1 = s.colbeg[c + 1];
        for (int64_t e = s.colbeg[c]; e < e1; ++e) {
            if (s.cells[e] == 0) continue;                             // (the same for every thread)
            const int64_t lo = s.lo[e], hi = s.hi[e];
            const double xv = EMIT ? xval[e] : 0.0;
            for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
                if (!((occ[i >> 6] >> (i & 63)) & 1ull)) continue;
                const int64_t row = keys[i];
                if (row == SEM_KEY) err |= SPG_ERR_STEP;
                else if (row < 1 || row > ny) err |= SPG_ERR_BOUNDS;
                else {
                    if (EMIT) acc[row - 1] = acc[row - 1] + xv * vals[i];
                    atomicOr(bm + ((row - 1) >> 6), 1ull << ((row - 1) & 63));
                }
            }
            if (EMIT) __syncthreads();                                 // the next entry adds to what this one stored
        }
        __syncthreads();
        if (!EMIT) {
            int64_t n = 0;
            for (int64_t w = threadIdx.x; w < nwords; w += 256) {
                const unsigned long long m = __hip_atomic_load(bm + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (m) { n += popc64(m); bm[w] = 0ull; }
            }
            n = wave_reduce_add(n);
            if (lane == 0) sSum[wv] = (unsigned long long)n;
            __syncthreads();
            if (threadIdx.x == 0) s.cnt[c] = (int64_t)(sSum[0] + sSum[1] + sSum[2] + sSum[3]);
            __syncthreads();
            continue;
        }
        const int64_t off = s.cnt[c], expect = s.cnt[c + 1] - off;
        int64_t run = 0;
        for (int64_t w0 = 0; w0 < nwords; w0 += 256) {
            const int64_t w = w0 + threadIdx.x;
            const unsigned long long myword = w < nwords ? __hip_atomic_load(bm + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
            const uint32_t pc = (uint32_t)popc64(myword);
            const uint32_t myoff = wave_excl_scan(pc);
            if (lane == 63) sSum[wv] = (unsigned long long)(myoff + pc);
            __syncthreads();
            int64_t wbase = run, tot = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) { const int64_t sq = (int64_t)sSum[q]; if (q < wv) wbase += sq; tot += sq; }
            uint64_t nz = __ballot(myword != 0ull);
            while (nz) {
                const int l = __ffsll((unsigned long long)nz) - 1;
                nz &= nz - 1;
                const unsigned long long mask = __shfl(myword, l, 64);
                const int64_t woff = wbase + (int64_t)__shfl(myoff, l, 64);
                if ((mask >> lane) & 1ull) {
                    const int64_t r = woff + popc64(mask & mask_lt(lane));
                    const int64_t row0 = ((w0 + wv * 64 + l) << 6) + lane;
                    const double v = acc[row0];
                    acc[row0] = 0.0;
                    if (r < expect) { spg_store_idx(yidx, off + r, row0 + 1, ix); yval[off + r] = v; }
                    else err |= SPG_ERR_STEP;
                }
            }
            if (myword != 0ull) bm[w] = 0ull;
            run += tot;
            __syncthreads();
        }
        if (run != expect) err |= SPG_ERR_STEP;
    }
    err = wave_or(err);
    if (lane == 0 && err) atomicOr(s.err, err);
}

// one workgroup: cnt becomes its exclusive prefix in place (cnt[k] = total), yptr[j] = base + cnt[j]
template <typename IT>
__global__ __launch_bounds__(EX_SCAN_THREADS) void k_spg_scan(SpgScratch s, int64_t k, int64_t base, IT* __restrict__ yptr,
                                                              unsigned long long* pinned, unsigned long long seq) {
    unsigned long long tot, tot2;
    block_excl_scan2(s.cnt, s.cnt, k,
                     [&](int64_t i, unsigned long long ro, unsigned long long) { s.cnt[i] = (int64_t)ro; yptr[i] = (IT)(base + (int64_t)ro); },
                     tot, tot2);
    if (threadIdx.x != 0) return;
    s.cnt[k] = (int64_t)tot;
    yptr[k] = (IT)(base + (int64_t)tot);
    hand_over(s.err, pinned, seq, 1, tot);
}

__global__ void k_spg_done(SpgScratch s, unsigned long long* pinned, unsigned long long seq) {
    hand_over(s.err, pinned, seq);
}

// ---- launches ---------------------------------------------------------------------------------------------------------------------
static bool spg_shape_ok(int64_t k, int64_t nnzx) { return k >= 0 && k <= INT32_MAX && nnzx >= 0 && nnzx <= INT32_MAX; }

hipError_t launch_spgemm_bound(const SlotView& V, SpgIndex ix, const void* d_xptr, const void* d_xidx, int64_t k, int64_t nnzx, void* scratch,
                               unsigned long long* pinned3, unsigned long long seq, hipStream_t stream) {
    if (V.capacity < 0 || V.table_len < 0 || !spg_shape_ok(k, nnzx)) return hipErrorInvalidValue;
    const SpgScratch s = spg_carve(scratch, k, nnzx);
    hipError_t e = hipMemsetAsync(scratch, 0, 16 + (size_t)k * 8, stream);
    if (e != hipSuccess) return e;
    const int64_t eblocks = (nnzx + 3) / 4, cblocks = (k + 1 + 255) / 256;
    const int64_t grid = eblocks + cblocks < SPG_GRID_MAX ? eblocks + cblocks : SPG_GRID_MAX;
    hipLaunchKernelGGL(k_spg_bound, dim3((unsigned)grid), dim3(256), 0, stream, V, ix, d_xptr, d_xidx, k, nnzx, s, eblocks, cblocks);
    hipLaunchKernelGGL(k_spg_classify, dim3(1), dim3(1024), 0, stream, s, k, pinned3, seq);
    return hipGetLastError();
}

hipError_t launch_spgemm_count(const SlotView& V, int64_t k, int64_t nnzx, int64_t ny, int64_t n_large, uint64_t* slabs,
                               int64_t nslabs, SpgIndex ix, void* d_yptr, void* scratch, unsigned long long* pinned3, unsigned long long seq,
                               hipStream_t stream) {
    if (!spg_shape_ok(k, nnzx) || ny < 0 || n_large < 0 || n_large > k || (n_large > 0 && (nslabs < 1 || !slabs))) return hipErrorInvalidValue;
    const SpgScratch s = spg_carve(scratch, k, nnzx);
    if (k > 0)
        hipLaunchKernelGGL(k_spg_lds<false>, dim3((unsigned)(k < SPG_GRID_MAX ? k : SPG_GRID_MAX)), dim3(64), 0, stream, V.keys, nullptr, V.occ, s,
                           nullptr, k, ny, ix, nullptr, nullptr);
    if (n_large > 0)
        hipLaunchKernelGGL(k_spg_slab<false>, dim3((unsigned)nslabs), dim3(256), 0, stream, V.keys, nullptr, V.occ, s, nullptr, ny,
                           reinterpret_cast<unsigned long long*>(slabs), spgemm_slab_words(ny), ix, nullptr, nullptr);
    if (ix.bits32)
        hipLaunchKernelGGL(k_spg_scan<int32_t>, dim3(1), dim3(EX_SCAN_THREADS), 0, stream, s, k, ix.base, static_cast<int32_t*>(d_yptr), pinned3, seq);
    else
        hipLaunchKernelGGL(k_spg_scan<int64_t>, dim3(1), dim3(EX_SCAN_THREADS), 0, stream, s, k, ix.base, static_cast<int64_t*>(d_yptr), pinned3, seq);
    return hipGetLastError();
}

hipError_t launch_spgemm_emit(const SlotView& V, const double* d_xval, int64_t k, int64_t nnzx, int64_t ny,
                              int64_t n_large, uint64_t* slabs, int64_t nslabs, SpgIndex ix, void* d_yidx, double* d_yval, void* scratch,
                              unsigned long long* pinned2, unsigned long long seq, hipStream_t stream) {
    if (!spg_shape_ok(k, nnzx) || k < 1 || ny < 1 || n_large < 0 || n_large > k || (n_large > 0 && (nslabs < 1 || !slabs)) || !d_yidx || !d_yval)
        return hipErrorInvalidValue;
    const SpgScratch s = spg_carve(scratch, k, nnzx);
    hipLaunchKernelGGL(k_spg_lds<true>, dim3((unsigned)(k < SPG_GRID_MAX ? k : SPG_GRID_MAX)), dim3(64), 0, stream, V.keys, V.vals, V.occ, s, d_xval, k,
                       ny, ix, d_yidx, d_yval);
    if (n_large > 0)
        hipLaunchKernelGGL(k_spg_slab<true>, dim3((unsigned)nslabs), dim3(256), 0, stream, V.keys, V.vals, V.occ, s, d_xval, ny,
                           reinterpret_cast<unsigned long long*>(slabs), spgemm_slab_words(ny), ix, d_yidx, d_yval);
    hipLaunchKernelGGL(k_spg_done, dim3(1), dim3(1), 0, stream, s, pinned2, seq);
    return hipGetLastError();
}

}  // namespace dsa
