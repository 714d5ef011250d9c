// csrc/assemble.hip — the fold in front of the general write from (row, column, value) triples in HBM (dsa_mat_assemble[_dev]): ANY
// triples — stored or not, repeated or not, in any order — become the distinct cells they address, each with ONE value, in (column,
// row) order; update.hip then writes the stored ones in place, the compaction here hands the others to insert.hip.
//
// Passes, all on the colmajor stream; the number of launches does not depend on n:
//   (sort)             launch_pair_sort of build.hip: the ops in (column, row, input order) with their input index.  The sort is
//                      STABLE: the ops of one cell are a run in ascending k, which is the whole basis of the fold's order
//   k_asm_flags<Head>  one lane per sorted position: head = (p2, k2) differs from the predecessor; one ballot word per wave, one
//                      count per tile of ASM_TILE positions
//   k_asm_scan         one workgroup: exclusive scan of the tile counts; the total m goes to pinned memory with the sequence number
//   k_asm_fold         the lane of each head: rank = tile prefix + heads of the tile in front of it; it walks its run in sorted
//                      order gathering V[idx[t]] — add: s = V[k1]; s = s + V[k2]; ... one IEEE add per op, the left fold of
//                      dynamicsparse over duplicates (src/pcsr.jl:374-375); set: the V of the run's last op, bits untouched — up
//                      to ASM_FOLD_INLINE ops; a longer run is queued
//   k_asm_fold_long    one wave per queued run: 64 coalesced idx loads, 64 gathers in flight, folded in order through shuffles
//   k_asm_flags<Miss>  the same flag pass over update's byte mask of the folded cells
//   k_asm_scan         (no hand-over: the host has the miss count from update's verdict)
//   k_asm_scatter      order-preserving compaction of the folded cells that are not stored
// k_asm_fold_long restates k_fold_long of build.hip: that one walks packed composites (key | partition | index in one word) and the
// builder's control block, neither of which exists behind the pair sort, so it cannot be shared without changing what build.hip
// compiles to.  The values are added in plain C++ under -ffp-contract=off; no float atomics anywhere, and the only integer atomic is
// the ticket of the long-run queue, whose order decides no bit of the result (every run writes its own rank).
// Not done here: insert.hip sorts the compacted misses again although they arrive in (column, row) order; reusing this sort inside
// insert's own is left for later.
#include "assemble.h"
#include "wave_dev.h"

namespace dsa {

constexpr int ASM_BLOCK = (int)ASM_TILE;       // one lane per position
constexpr int ASM_WAVES = ASM_BLOCK / 64;

// ---- the two flag sources of the tile machinery
struct AsmHeadFlag {      // sorted position t starts a run of equal cells
    const int64_t* p2; const int64_t* k2;
    __device__ __forceinline__ bool operator()(int64_t t) const { return t == 0 || p2[t] != p2[t - 1] || k2[t] != k2[t - 1]; }
};
struct AsmMissFlag {      // folded cell t is not stored
    const uint8_t* miss;
    __device__ __forceinline__ bool operator()(int64_t t) const { return miss[t] != 0; }
};

// flags -> one ballot word per wave, one count per tile
template <typename Flag>
__global__ __launch_bounds__(ASM_BLOCK) void k_asm_flags(Flag flag, int64_t n, uint64_t* __restrict__ words, uint32_t* __restrict__ tcnt) {
    __shared__ uint32_t cnt[ASM_WAVES];
    const int64_t t = (int64_t)blockIdx.x * ASM_TILE + threadIdx.x;
    const int wv = threadIdx.x >> 6;
    const uint64_t w = __ballot(t < n && flag(t));
    if (lane_id() == 0) {
        if ((t >> 6) < ((n + 63) >> 6)) words[t >> 6] = w;
        cnt[wv] = (uint32_t)popc64(w);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t c = 0;
        for (int q = 0; q < ASM_WAVES; ++q) c += cnt[q];
        tcnt[blockIdx.x] = c;
    }
}

// exclusive scan of the tile counts by one workgroup: every thread a contiguous chunk
__global__ __launch_bounds__(1024) void k_asm_scan(const uint32_t* __restrict__ tcnt, uint32_t* __restrict__ toff, int64_t tiles,
                                                  unsigned long long* __restrict__ hdr, unsigned long long* pinned, unsigned long long seq) {
    __shared__ uint32_t wsum[16];
    const int64_t chunk = (tiles + 1023) / 1024;
    const int64_t lo = (int64_t)threadIdx.x * chunk, hi = lo + chunk < tiles ? lo + chunk : tiles;
    uint32_t s = 0;
    for (int64_t q = lo; q < hi; ++q) s += tcnt[q];
    const uint32_t in_wave = wave_excl_scan(s);
    const int wv = threadIdx.x >> 6;
    if (lane_id() == 63) wsum[wv] = in_wave + s;
    __syncthreads();
    uint32_t base = in_wave;
    for (int q = 0; q < wv; ++q) base += wsum[q];
    for (int64_t q = lo; q < hi; ++q) { toff[q] = base; base += tcnt[q]; }
    if (threadIdx.x == 1023) {
        hdr[1] = base;
        if (pinned != nullptr) {
            __hip_atomic_store(pinned, (unsigned long long)base, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            publish_seq(pinned + ASM_PIN_WORDS - 1, seq);
        }
    }
}

// the 0-based rank of the flagged position of this lane among all flagged positions; called by every thread of the workgroup
__device__ __forceinline__ uint32_t asm_rank(uint64_t word, const uint32_t* __restrict__ toff, uint32_t* cnt) {
    const int wv = threadIdx.x >> 6;
    if (lane_id() == 0) cnt[wv] = (uint32_t)popc64(word);
    __syncthreads();
    uint32_t r = toff[blockIdx.x];
    for (int q = 0; q < wv; ++q) r += cnt[q];
    return r + (uint32_t)popc64(word & mask_lt(lane_id()));
}

__device__ __forceinline__ bool asm_bit(const uint64_t* __restrict__ words, int64_t t) { return (words[t >> 6] >> (t & 63)) & 1ull; }

__global__ __launch_bounds__(ASM_BLOCK) void k_asm_fold(const uint64_t* __restrict__ words, const uint32_t* __restrict__ toff, const uint32_t* __restrict__ idx,
                                                       const int64_t* __restrict__ k2, const int64_t* __restrict__ p2, const double* __restrict__ V,
                                                       int64_t n, bool add, int64_t* __restrict__ fI, int64_t* __restrict__ fJ,
                                                       double* __restrict__ fV, uint32_t* __restrict__ flast, unsigned long long* __restrict__ hdr,
                                                       AsmLongRun* __restrict__ queue) {
    __shared__ uint32_t cnt[ASM_WAVES];
    const int64_t t = (int64_t)blockIdx.x * ASM_TILE + threadIdx.x;
    const uint64_t word = t < n ? words[t >> 6] : 0ull;
    const uint32_t rank = asm_rank(word, toff, cnt);
    if (t >= n || !((word >> lane_id()) & 1ull)) return;
    fI[rank] = k2[t];
    fJ[rank] = p2[t];
    double acc = add ? V[idx[t]] : 0.0;
    int64_t u = t + 1;
    int len = 1;
    while (u < n && len < ASM_FOLD_INLINE && !asm_bit(words, u)) {
        if (add) acc = acc + V[idx[u]];
        ++u; ++len;
    }
    if (u < n && !asm_bit(words, u)) {      // more than ASM_FOLD_INLINE ops: a wave finishes the run
        const unsigned long long q = atomicAdd(&hdr[0], 1ull);
        AsmLongRun lr; lr.next = u; lr.rank = (int64_t)rank; lr.acc = acc;
        queue[q] = lr;
        return;
    }
    const uint32_t last = idx[u - 1];
    fV[rank] = add ? acc : V[last];
    flast[rank] = last;
}

__global__ __launch_bounds__(64) void k_asm_fold_long(const uint64_t* __restrict__ words, const uint32_t* __restrict__ idx, const double* __restrict__ V,
                                                     int64_t n, bool add, const unsigned long long* __restrict__ hdr,
                                                     const AsmLongRun* __restrict__ queue, double* __restrict__ fV, uint32_t* __restrict__ flast) {
    const int lane = threadIdx.x;
    const unsigned long long nl = hdr[0];
    for (unsigned long long q = blockIdx.x; q < nl; q += gridDim.x) {
        const AsmLongRun lr = queue[q];
        double acc = lr.acc;
        int64_t t = lr.next;          // (the run has at least one op here)
        uint32_t last = 0;
        while (true) {
            const int64_t i = t + lane;
            const bool same = i < n && !asm_bit(words, i);
            const uint32_t src = i < n ? idx[i] : 0u;
            const double v = same ? V[src] : 0.0;
            const uint64_t b = __ballot(same);
            const int cnt = b == ~0ull ? 64 : __ffsll((unsigned long long)~b) - 1;      // the ops in front of the next head
            if (add) {
                for (int l = 0; l < cnt; ++l) acc = acc + __shfl(v, l, 64);
            } else if (cnt > 0) {
                acc = __shfl(v, cnt - 1, 64);
            }
            if (cnt > 0) last = readlane32(src, cnt - 1);
            if (cnt < 64) break;
            t += 64;
        }
        if (lane == 0) { fV[lr.rank] = acc; flast[lr.rank] = last; }
    }
}

__global__ __launch_bounds__(ASM_BLOCK) void k_asm_scatter(const uint64_t* __restrict__ words, const uint32_t* __restrict__ toff, int64_t m,
                                                          const int64_t* __restrict__ fI, const int64_t* __restrict__ fJ, const double* __restrict__ fV,
                                                          const uint32_t* __restrict__ flast, int64_t* __restrict__ cI, int64_t* __restrict__ cJ,
                                                          double* __restrict__ cV, uint32_t* __restrict__ clast) {
    __shared__ uint32_t cnt[ASM_WAVES];
    const int64_t t = (int64_t)blockIdx.x * ASM_TILE + threadIdx.x;
    const uint64_t word = t < m ? words[t >> 6] : 0ull;
    const uint32_t rank = asm_rank(word, toff, cnt);
    if (t >= m || !((word >> lane_id()) & 1ull)) return;
    cI[rank] = fI[t];
    cJ[rank] = fJ[t];
    cV[rank] = fV[t];
    clast[rank] = flast[t];
}

hipError_t launch_assemble_fold(const int64_t* d_I, const int64_t* d_J, const double* d_V, int64_t n, int64_t imin, int ibits, int64_t jmin,
                                int jbits, bool add, void* scratch, unsigned long long* pinned, unsigned long long seq, hipStream_t stream) {
    if (n < 1 || n > (int64_t)INT32_MAX) return hipErrorInvalidValue;
    const AsmScratch s = asm_carve(scratch, n);
    hipError_t e = hipMemsetAsync(s.hdr, 0, 256, stream);
    if (e != hipSuccess) return e;
    // colmajor order: the partitions are the columns, the inner keys the rows
    e = launch_pair_sort(d_J, d_I, n, jmin, jbits, imin, ibits, s.sort, s.idx, s.k2, s.p2, stream);
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)s.tiles), block(ASM_BLOCK);
    hipLaunchKernelGGL(k_asm_flags<AsmHeadFlag>, grid, block, 0, stream, AsmHeadFlag{s.p2, s.k2}, n, s.words, s.tcnt);
    hipLaunchKernelGGL(k_asm_scan, dim3(1), dim3(1024), 0, stream, (const uint32_t*)s.tcnt, s.toff, s.tiles, s.hdr, pinned, seq);
    hipLaunchKernelGGL(k_asm_fold, grid, block, 0, stream, (const uint64_t*)s.words, (const uint32_t*)s.toff, (const uint32_t*)s.idx,
                       (const int64_t*)s.k2, (const int64_t*)s.p2, d_V, n, add, s.fI, s.fJ, s.fV, s.flast, s.hdr, s.queue);
    hipLaunchKernelGGL(k_asm_fold_long, dim3(ASM_LONG_BLOCKS), dim3(64), 0, stream, (const uint64_t*)s.words, (const uint32_t*)s.idx, d_V, n, add,
                       (const unsigned long long*)s.hdr, (const AsmLongRun*)s.queue, s.fV, s.flast);
    return hipGetLastError();
}

hipError_t launch_assemble_compact(void* scratch, int64_t n, int64_t m, hipStream_t stream) {
    if (m < 1 || m > n) return hipErrorInvalidValue;
    const AsmScratch s = asm_carve(scratch, n);
    const int64_t tiles = asm_tiles(m);
    const dim3 grid((unsigned)tiles), block(ASM_BLOCK);
    hipLaunchKernelGGL(k_asm_flags<AsmMissFlag>, grid, block, 0, stream, AsmMissFlag{s.miss}, m, s.words, s.tcnt);
    hipLaunchKernelGGL(k_asm_scan, dim3(1), dim3(1024), 0, stream, (const uint32_t*)s.tcnt, s.toff, tiles, s.hdr, (unsigned long long*)nullptr, 0ull);
    hipLaunchKernelGGL(k_asm_scatter, grid, block, 0, stream, (const uint64_t*)s.words, (const uint32_t*)s.toff, m, (const int64_t*)s.fI,
                       (const int64_t*)s.fJ, (const double*)s.fV, (const uint32_t*)s.flast, s.cI, s.cJ, s.cV, s.clast);
    return hipGetLastError();
}

}  // namespace dsa
