// csrc/vecops.hip — whole-vector operations on the PACKED cells of a DynamicSparseVector, on gfx950: the two-stage reductions behind
// dsa_vec_reduce (sum, sum |v|, sum v*v, max |v|), dsa_vec_dot (sparse . sparse) and dsa_vec_dot_dense_dev (sparse . dense), the
// copy-out of packed cells with the keys widened to int64 (dsa_vec_nonzeros_dev; the x of dsa_mat_mul_vec), and the scatter of
// dsa_vec_to_dense_dev.  Host side: vecops_host.hip.
//
// Everything here reads the output of K-pack (the alternate slot buffer of a vector: ascending, distinct keys in their physical
// width, values beside them), never the slot array: what a reduction returns depends on the stored (key, value) pairs only, not on
// where the cells sit — two vectors with v1 == v2 give the same bits.
//
// Reduction = two kernels, one pair for every term (VoTerm, vecops.h):
//   k_vec_terms<TERM>   one lane per packed cell of the driving operand, coalesced (key in its physical width + value).  VO_DOT
//                       looks the lane's key up in the other operand with packed_bound (wave_dev.h, the bisection of
//                       k_merge_axpby): ceil(log2(nb + 1)) DEPENDENT key loads per lane, served by L2 after the first lanes have
//                       walked the top of the tree, then one value load on a hit; a miss contributes +0.0.  VO_DOT_DENSE gathers
//                       x[key - 1] and checks the key against 1..nx in the same pass.  Lanes behind the last cell contribute +0.0.
//                       The wave joins its 64 terms in the xor butterfly o = 32 .. 1 (addition commutes bit for bit, so every lane
//                       holds the same word) and lane 0 stores ONE partial.
//   k_vec_finish<MAX>   one workgroup of VO_FIN_THREADS: thread t joins the partials t, t + VO_FIN_THREADS, ... in index order
//                       (one pass per VO_FIN_THREADS partials = VO_PASS_CELLS driving cells), the butterfly joins the threads of a
//                       wave, wave 0 joins the 16 wave words the same way; thread 0 stores the scalar and the error word and hands
//                       both to the host through pinned words (no copy command).
// No floating-point atomics: the order of every addition is a function of the packed index alone, two calls give the same bits.
// Products and sums are rounded separately (__dmul_rn / __dadd_rn).  VO_SQSUM's term is __dmul_rn(v, v) and VO_DOT of a vector
// with itself multiplies the same two words in the same lane: dsa_vec_dot(a, a) and the sum of squares are the same bits.  Every
// accumulator starts at +0.0 and every wave is padded with +0.0, so an empty vector gives +0.0 and a sum of negative zeros is +0.0.
// VO_ABSMAX compares the bit patterns of |v| as unsigned integers (NaN is above Inf and propagates, as in scale.hip).
// Bytes per call: driving operand 12 | 16 B per cell (int32 | int64 keys) read once; VO_DOT adds the bisection (L2-resident top of
// the other operand's key array, its leaves once: at most 4 | 8 B x nb of HBM traffic) and 8 B per hit; VO_DOT_DENSE one 8 B gather
// per cell; 8 B written per 64 cells, read once by stage 2.  A merge-path partition for operands of similar length (one pass over
// both instead of na bisections) is not built.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; no scratch in any kernel, occupancy 8 waves per SIMD everywhere):
//   k_vec_terms     SUM / ABSSUM / SQSUM 10 VGPRs (ABSMAX 9), 12 SGPRs; DOT 16 VGPRs, 27 SGPRs; DOT_DENSE 12 VGPRs, 20 SGPRs;
//                   BOUNDS 6 VGPRs, 17 SGPRs; no LDS
//   k_vec_finish    13 VGPRs (ABSMAX 14), 22 SGPRs, 128 B LDS (the 16 wave words)
//   k_vec_copy_out  16 VGPRs, 38 SGPRs, no LDS;  k_vec_scatter 12 VGPRs, 28 SGPRs, no LDS
#include "vecops.h"
#include "wave_dev.h"
#include <algorithm>

namespace dsa {

template <int TERM>
__device__ __forceinline__ double vo_join(double a, double b) {
    if (TERM == VO_ABSMAX) return (uint64_t)__double_as_longlong(b) > (uint64_t)__double_as_longlong(a) ? b : a;
    return __dadd_rn(a, b);
}
// the join of a wave's 64 words in a fixed tree; every lane returns the same word
template <int TERM>
__device__ __forceinline__ double vo_wave_join(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = vo_join<TERM>(v, __shfl_xor(v, o, 64));
    return v;
}

// ---- stage 1 ---------------------------------------------------------------------------------------------------------------------
template <int TERM>
__global__ __launch_bounds__(VO_BLOCK) void k_vec_terms(KeyArr ka, const double* __restrict__ va, int64_t na, KeyArr kb,
                                                        const double* __restrict__ vb, int64_t nb, const double* __restrict__ xd,
                                                        int64_t nx, double* __restrict__ partial, unsigned int* __restrict__ errw) {
    const int64_t i = (int64_t)blockIdx.x * VO_BLOCK + threadIdx.x;
    double term = 0.0;
    bool outside = false;
    if (i < na) {
        if (TERM == VO_SUM) term = va[i];
        else if (TERM == VO_ABSSUM || TERM == VO_ABSMAX) term = fabs(va[i]);
        else if (TERM == VO_SQSUM) { const double v = va[i]; term = __dmul_rn(v, v); }
        else if (TERM == VO_DOT) {
            const int64_t key = ka[i];
            const int64_t lb = packed_bound(kb, nb, key, false);
            if (lb < nb && kb[lb] == key) term = __dmul_rn(va[i], vb[lb]);
        } else {
            const int64_t key = ka[i];
            outside = key < 1 || key > nx;
            if (TERM == VO_DOT_DENSE && !outside) term = __dmul_rn(va[i], xd[key - 1]);
        }
    }
    if (TERM == VO_DOT_DENSE || TERM == VO_BOUNDS) {
        if (__ballot(outside) != 0ull && (threadIdx.x & 63) == 0) atomicOr(errw, 1u);
    }
    term = vo_wave_join<TERM>(term);
    if ((threadIdx.x & 63) == 0 && i < na) partial[i >> 6] = term;          // (a wave wholly behind the last cell has no partial)
}

// ---- stage 2 ---------------------------------------------------------------------------------------------------------------------
template <int TERM>
__global__ __launch_bounds__(VO_FIN_THREADS) void k_vec_finish(const double* __restrict__ partial, int64_t np, unsigned long long* __restrict__ hdr,
                                                              unsigned long long* __restrict__ pin, unsigned long long seq) {
    __shared__ double sWave[VO_FIN_THREADS / 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double acc = 0.0;
    for (int64_t p = threadIdx.x; p < np; p += VO_FIN_THREADS) acc = vo_join<TERM>(acc, partial[p]);
    acc = vo_wave_join<TERM>(acc);
    if (lane == 0) sWave[wv] = acc;
    __syncthreads();
    if (wv != 0) return;
    double w = lane < VO_FIN_THREADS / 64 ? sWave[lane] : 0.0;
    w = vo_wave_join<TERM>(w);
    if (lane == 0) {
        const unsigned long long bits = (unsigned long long)__double_as_longlong(w);
        const unsigned long long err = (unsigned long long)*reinterpret_cast<const unsigned int*>(hdr + 1);
        hdr[0] = bits;
        __hip_atomic_store(pin + VO_PIN_RESULT, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(pin + VO_PIN_ERR, err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        publish_seq(pin + VO_PIN_SEQ, seq);
    }
}

hipError_t launch_vec_reduce(int32_t term, KeyArr ka, const double* va, int64_t na, KeyArr kb, const double* vb, int64_t nb,
                             const double* xd, int64_t nx, void* scratch, unsigned long long* pin, unsigned long long seq,
                             hipStream_t stream) {
    unsigned long long* hdr = static_cast<unsigned long long*>(scratch);
    double* partial = reinterpret_cast<double*>(static_cast<char*>(scratch) + 64);
    unsigned int* errw = reinterpret_cast<unsigned int*>(hdr + 1);
    const int64_t np = vo_partials(na);
    hipError_t e = hipMemsetAsync(hdr, 0, 64, stream);
    if (e != hipSuccess) return e;
    const unsigned grid = (unsigned)((na + VO_BLOCK - 1) / VO_BLOCK);
#define DSA_VO_CASE(T_) case T_: if (grid) hipLaunchKernelGGL((k_vec_terms<T_>), dim3(grid), dim3(VO_BLOCK), 0, stream, ka, va, na, kb, vb, nb, xd, nx, partial, errw); break
    switch (term) {
        DSA_VO_CASE(VO_SUM); DSA_VO_CASE(VO_ABSSUM); DSA_VO_CASE(VO_SQSUM); DSA_VO_CASE(VO_ABSMAX);
        DSA_VO_CASE(VO_DOT); DSA_VO_CASE(VO_DOT_DENSE); DSA_VO_CASE(VO_BOUNDS);
        default: return hipErrorInvalidValue;
    }
#undef DSA_VO_CASE
    if (term == VO_ABSMAX) hipLaunchKernelGGL((k_vec_finish<VO_ABSMAX>), dim3(1), dim3(VO_FIN_THREADS), 0, stream, partial, np, hdr, pin, seq);
    else hipLaunchKernelGGL((k_vec_finish<VO_SUM>), dim3(1), dim3(VO_FIN_THREADS), 0, stream, partial, np, hdr, pin, seq);
    return hipGetLastError();
}

// ---- copy-out: packed cells -> int64 keys + values ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_vec_copy_out(KeyArr k, const double* __restrict__ v, int64_t n, int64_t* __restrict__ out_k,
                                                      double* __restrict__ out_v, unsigned long long* __restrict__ pin, unsigned long long seq) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const int64_t key = k[i];
        out_k[i] = key; out_v[i] = v[i];
        if (i == 0 && pin != nullptr) {
            __hip_atomic_store(pin + VO_PIN_FIRST, (unsigned long long)key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            publish_seq(pin + VO_PIN_SEQ, seq);
        }
    }
}
hipError_t launch_vec_copy_out(KeyArr k, const double* v, int64_t n, int64_t* out_k, double* out_v, unsigned long long* pin,
                               unsigned long long seq, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    const int blocks = (int)std::min<int64_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(k_vec_copy_out, dim3(blocks), dim3(256), 0, stream, k, v, n, out_k, out_v, pin, seq);
    return hipGetLastError();
}

// ---- densify: x[key - 1] = value (the host has the bounds verdict before it enqueues this; the guard costs nothing) ----------------
__global__ __launch_bounds__(256) void k_vec_scatter(KeyArr k, const double* __restrict__ v, int64_t n, double* __restrict__ x, int64_t nx) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const int64_t key = k[i];
        if (key >= 1 && key <= nx) x[key - 1] = v[i];
    }
}
hipError_t launch_vec_scatter(KeyArr k, const double* v, int64_t n, double* x, int64_t nx, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    const int blocks = (int)std::min<int64_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(k_vec_scatter, dim3(blocks), dim3(256), 0, stream, k, v, n, x, nx);
    return hipGetLastError();
}

}  // namespace dsa
