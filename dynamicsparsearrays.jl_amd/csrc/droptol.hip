// csrc/droptol.hip — K-droptol: every stored cell whose value is small leaves both orientations of a matrix in place
// (dsa_mat_droptol[_dev]; SparseArrays' dropzeros! / droptol!, and what the reference's setindex! with a zero does for one cell,
// src/matrix.jl:43-62).  A cell (i, j) with value v is dropped iff |v| <= tol, or |v| <= tr[i - 1], or |v| <= tc[j - 1] (IEEE
// comparisons: a NaN value is never dropped, a NaN or negative threshold matches nothing, -0.0 is zero).  The kernels only clear
// occupancy bits: the pack + spread of the survivors is the root rebalance the host enqueues behind them (rebalance.hip), so keys and
// values are never touched, and a semaphore slot is never cleared — a partition that loses its last cell stays as an empty one.
//
// Two passes per orientation, on the orientation's stream; the number of launches does not depend on the matrix or on the count:
//   (launch_scale_check of scale.hip, only with a threshold vector: the bounds word and per span the partition open at its start)
//   k_drop_decide  the spans of scale.hip: one wave per 512 slots (8 occupancy words), lane <-> slot, the words, keys and values of
//                  the span requested before anything waits.  A lane holds a cell iff its slot is occupied and its key is not SEM_KEY.
//                  With a vector it gathers t_key[key - 1], and the threshold of its partition comes from the nearest semaphore at
//                  or below its lane (t_part[part_keys[id - 1] - 1], handed on by a shuffle), in front of the word's first semaphore
//                  from the partition that is open — the carry of k_scale.  An absent threshold is -1.0: |v| <= -1 is never true.
//                  The ballot of the predicate is the word's DROP MASK, stored by lane 0 (one 8-byte entry per occupancy word, zero
//                  words included: pass 2 reads every one); the popcounts of the span go into the span's own counter, a plain store
//                  (one atomic per wave on a common counter serialises in the L2: with 1 % of the cells of 2^24 slots dropped
//                  nearly every one of the 32768 waves has something to add, and the pass took 594 us instead of 34).
//   k_drop_verdict one workgroup: the sum of the span counters (integers, fixed order), {error word, count, seq} to pinned memory
//   (host: waits for both orientations; the counts must agree; nothing to drop or count-only: done, nothing was written)
//   k_drop_mark    one thread per occupancy word: occ[w] &= ~mask[w], a plain store by the word's only writer.  The predicate is
//                  evaluated once, in pass 1: the two passes cannot disagree.
// Which bits are cleared is a function of the values and thresholds alone and the count is an integer sum: the same input gives the
// same bits on every call, no atomics at all.
// Bytes per orientation: occupancy + keys + values read once = 12.1 B (int32 keys) | 16.1 B (int64 keys) per slot; with a vector the
// check's 4.1 | 8.1 B per slot + 16 B per span, and the gathers; the masks 0.125 B per slot written and read again, 4 B per span of counters.
// Slot loads go around the cache when the slot array does not fit an XCD's L2 beside the vectors (nt), as in scale.hip.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; no scratch, occupancy 8 waves per SIMD in every kernel):
//   k_drop_decide  scalar form 32 VGPRs (int64 keys 42), 66 SGPRs; with a vector 57 VGPRs, 84 SGPRs in all four instantiations; no LDS
//   k_drop_verdict 10 VGPRs, 22 SGPRs, 8192 B LDS (one workgroup);  k_drop_mark 6 VGPRs, 12 SGPRs, no LDS
#include "droptol.h"
#include "scale.h"
#include "scale_dev.h"

namespace dsa {

constexpr int DR_SUM_THREADS = 1024;

static inline size_t dr_head_bytes(int64_t capacity) { return (scale_scratch_bytes(capacity) + 15) & ~(size_t)15; }
static inline size_t dr_count_bytes(int64_t capacity) { return ((size_t)sc_spans(capacity) * sizeof(uint32_t) + 15) & ~(size_t)15; }
size_t droptol_scratch_bytes(int64_t capacity) {
    return dr_head_bytes(capacity) + dr_count_bytes(capacity) + (size_t)((capacity + 63) >> 6) * sizeof(uint64_t);
}
struct DrScratch {
    ScScratch sc; uint32_t* counts; uint64_t* masks;      // one counter per span, one mask per occupancy word
    DrScratch(void* scratch, int64_t capacity) : sc(scratch, capacity) {
        char* p = static_cast<char*>(scratch) + dr_head_bytes(capacity);
        counts = reinterpret_cast<uint32_t*>(p);
        masks = reinterpret_cast<uint64_t*>(p + dr_count_bytes(capacity));
    }
};

// t_part[part_key(id) - 1], or -1.0 (matches nothing) when the vector is absent or the id / key is not usable (the check pass reports that)
__device__ __forceinline__ double dr_part_thr(int64_t id, const int64_t* __restrict__ part_keys, int64_t table_len,
                                              const double* __restrict__ t_part, int64_t dim_part) {
    if (t_part == nullptr || id < 1 || id > table_len) return -1.0;
    const int64_t key = part_keys[id - 1];
    return key >= 1 && key <= dim_part ? t_part[key - 1] : -1.0;
}

template <bool WIDE, bool NT, bool VEC>
__global__ __launch_bounds__(SC_BLOCK) void k_drop_decide(KeyArr keys, const double* __restrict__ vals, const uint64_t* __restrict__ occ,
                                                          int64_t capacity, const int64_t* __restrict__ part_keys, int64_t table_len, double tol,
                                                          const double* __restrict__ t_key, int64_t dim_key, const double* __restrict__ t_part,
                                                          int64_t dim_part, const int64_t* __restrict__ carry, uint64_t* __restrict__ masks,
                                                          uint32_t* __restrict__ counts) {
    typedef typename std::conditional<WIDE, int64_t, int32_t>::type key_t;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t nwords = (capacity + 63) >> 6;
    const int64_t span = (int64_t)blockIdx.x * SC_WAVES + wv;
    const int64_t w0 = span * SC_WORDS;
    if (w0 >= nwords) return;                             // whole waves: nothing below waits for another wave
    uint64_t ow[SC_WORDS];
    key_t k[SC_WORDS];
    double v[SC_WORDS];
    sc_load_span<WIDE, NT, true>(static_cast<const key_t*>(keys.p), vals, occ, nwords, w0, lane, ow, k, v);

    uint64_t drop[SC_WORDS];
    if (VEC) {
        const uint64_t udim = (uint64_t)(dim_key > 0 ? dim_key : 0);
        double open_t = dr_part_thr(carry[span], part_keys, table_len, t_part, dim_part);      // wave-uniform: the open partition's threshold
        // the gathers of the whole span are requested before the first comparison waits for one
        double tk[SC_WORDS], ts[SC_WORDS];
        bool cell[SC_WORDS];
        uint64_t sbs[SC_WORDS];
#pragma unroll
        for (int j = 0; j < SC_WORDS; ++j) {
            const bool here = (ow[j] >> lane) & 1ull;
            const bool issem = here && k[j] == (key_t)SEM_KEY;
            sbs[j] = __ballot(issem);
            cell[j] = here && !issem;
            tk[j] = (cell[j] && t_key != nullptr && (uint64_t)((int64_t)k[j] - 1) < udim) ? t_key[(int64_t)k[j] - 1] : -1.0;
            ts[j] = issem ? dr_part_thr((int64_t)v[j], part_keys, table_len, t_part, dim_part) : -1.0;
        }
#pragma unroll
        for (int j = 0; j < SC_WORDS; ++j) {
            const uint64_t sb = sbs[j];
            const uint64_t below = sb & mask_le(lane);
            const double tl = __shfl(ts[j], below ? top_bit(below) : 0, 64);
            const double tp = below ? tl : open_t;
            const double a = fabs(v[j]);
            drop[j] = __ballot(cell[j] && (a <= tol || a <= tk[j] || a <= tp));
            if (sb != 0ull) open_t = readlane_f64(ts[j], top_bit(sb));
        }
    } else {
#pragma unroll
        for (int j = 0; j < SC_WORDS; ++j) {
            const bool here = (ow[j] >> lane) & 1ull;
            drop[j] = __ballot(here && k[j] != (key_t)SEM_KEY && fabs(v[j]) <= tol);
        }
    }
    uint32_t cnt = 0;                                     // wave-uniform, <= 512
#pragma unroll
    for (int j = 0; j < SC_WORDS; ++j) {
        if (lane == 0 && w0 + j < nwords) masks[w0 + j] = drop[j];
        cnt += (uint32_t)popc64(drop[j]);
    }
    if (lane == 0) counts[span] = cnt;                    // every span stores its counter: nothing to clear in front
}

// one workgroup, behind the check pass (if any) and k_drop_decide on the stream: the span counters summed in a fixed order
__global__ __launch_bounds__(DR_SUM_THREADS) void k_drop_verdict(const ScHeader* __restrict__ sc, const uint32_t* __restrict__ counts,
                                                                 int64_t nspans, unsigned long long* pinned, unsigned long long seq) {
    __shared__ unsigned long long sC[DR_SUM_THREADS];
    const int t = threadIdx.x;
    unsigned long long c = 0;
    for (int64_t s = t; s < nspans; s += DR_SUM_THREADS) c += counts[s];
    sC[t] = c;
    __syncthreads();
    for (int o = DR_SUM_THREADS / 2; o > 0; o >>= 1) {
        if (t < o) sC[t] += sC[t + o];
        __syncthreads();
    }
    if (t != 0) return;
    const uint32_t e = __hip_atomic_load(&sc->err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(pinned + 0, (unsigned long long)e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(pinned + 1, sC[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    publish_seq(pinned + 2, seq);
}

// every thread owns whole words: plain stores
__global__ __launch_bounds__(SC_BLOCK) void k_drop_mark(uint64_t* __restrict__ occ, const uint64_t* __restrict__ masks, int64_t nwords) {
    const int64_t w = (int64_t)blockIdx.x * SC_BLOCK + threadIdx.x;
    if (w >= nwords) return;
    const uint64_t m = masks[w];
    if (m != 0ull) occ[w] &= ~m;
}

// ---- launch wrappers -----------------------------------------------------------------------------------------------------------
hipError_t launch_droptol_decide(const SlotView& V, double tol, const double* t_key, int64_t dim_key, const double* t_part, int64_t dim_part,
                                 bool nt, void* scratch, unsigned long long* pinned, unsigned long long seq, hipStream_t stream) {
    if (V.capacity <= 0) return hipErrorInvalidValue;
    const DrScratch S(scratch, V.capacity);
    const bool vec = t_key != nullptr || t_part != nullptr;
    hipError_t e;
    if (vec) e = launch_scale_check(V, dim_key, dim_part, scratch, pinned + 3, seq, stream);      // clears the bounds word, leaves the carry
    else e = hipMemsetAsync(S.sc.hdr, 0, sizeof(ScHeader), stream);
    if (e != hipSuccess) return e;
    const unsigned grid = (unsigned)((S.sc.nspans + SC_WAVES - 1) / SC_WAVES);
    const int64_t* carry = static_cast<const int64_t*>(S.sc.a1);
#define DSA_DROP_CASE(W_, N_, V_) hipLaunchKernelGGL((k_drop_decide<W_, N_, V_>), dim3(grid), dim3(SC_BLOCK), 0, stream, V.keys, V.vals, V.occ, V.capacity, \
                                                     V.part_keys, V.table_len, tol, t_key, dim_key, t_part, dim_part, carry, S.masks, S.counts)
    switch ((V.keys.wide ? 4 : 0) | (nt ? 2 : 0) | (vec ? 1 : 0)) {
        case 0: DSA_DROP_CASE(false, false, false); break;
        case 1: DSA_DROP_CASE(false, false, true); break;
        case 2: DSA_DROP_CASE(false, true, false); break;
        case 3: DSA_DROP_CASE(false, true, true); break;
        case 4: DSA_DROP_CASE(true, false, false); break;
        case 5: DSA_DROP_CASE(true, false, true); break;
        case 6: DSA_DROP_CASE(true, true, false); break;
        default: DSA_DROP_CASE(true, true, true); break;
    }
#undef DSA_DROP_CASE
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_drop_verdict, dim3(1), dim3(DR_SUM_THREADS), 0, stream, S.sc.hdr, S.counts, S.sc.nspans, pinned, seq);
    return hipGetLastError();
}

hipError_t launch_droptol_mark(uint64_t* occ, int64_t capacity, const void* scratch, hipStream_t stream) {
    if (capacity <= 0 || !occ) return hipErrorInvalidValue;
    const DrScratch S(const_cast<void*>(scratch), capacity);
    const int64_t nwords = (capacity + 63) >> 6;
    hipLaunchKernelGGL(k_drop_mark, dim3((unsigned)((nwords + SC_BLOCK - 1) / SC_BLOCK)), dim3(SC_BLOCK), 0, stream, occ, S.masks, nwords);
    return hipGetLastError();
}

}  // namespace dsa
