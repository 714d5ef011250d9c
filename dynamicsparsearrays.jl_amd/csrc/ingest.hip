// csrc/ingest.hip — K-ingest: COO / CSR / CSC arrays that are already in HBM become the 1-based int64 (row, column) keys K-build sorts
// (build.hip reads them as it reads an upload).  Values are never touched: the builder gathers them from the caller's array.
//   k_in_init     the five running words {a min, a max, b min, b max, flags}
//   k_in_expand   ptr -> one outer key per entry.  Work is cut by ENTRIES into items of IN_ITEM: an item bisects ptr for the slice of its
//                 first and of its last entry, its threads bisect only between those two — a slice of 10^7 entries is shared by 5000
//                 items, a run of empty slices is stepped over by the bisection and costs its ptr words in the check.  The same launch
//                 checks ptr: both ends against base and base + nnz, every step non-decreasing.  The outer range is the slice of the
//                 first and of the last entry.
//   k_in_keys     idx (the COO arrays when they are not 64-bit, 1-based already) -> keys, and in the same pass what k_minmax computes
//                 for an upload: min, max and the reserved key 0 per array.  The range check of a compressed inner index against
//                 `inner` is the host's comparison of that min / max with 1 and inner.
//   k_in_publish  the five words to pinned memory, then the sequence number: the one wait of the host.
// Bytes, compressed with ib-byte indices: ib * (outer + 1) (twice through the cache: the check reads the neighbour, the bisections hit
// L2) + ib * nnz in, 16 * nnz out.  One atomic per workgroup and word; none on the entry stream.
#include "ingest.h"
#include "wave_dev.h"
#include <algorithm>
#include <climits>

namespace dsa {

__global__ void k_in_init(long long* __restrict__ acc) {
    if (threadIdx.x == 0) { acc[0] = INT64_MAX; acc[1] = INT64_MIN; acc[2] = INT64_MAX; acc[3] = INT64_MIN; acc[4] = 0; }
}

// the slice of entry p: the largest j in [lo, hi] with ptr[j] - base <= p (empty slices in front of it share its ptr value and lose)
template <typename IT>
__device__ __forceinline__ int64_t in_slice_of(const IT* __restrict__ ptr, int64_t base, int64_t p, int64_t lo, int64_t hi) {
    // CLAMP: a ptr that has not been checked yet (the check runs in this very launch) is only ever COMPARED here, never used as an
    // address.  Every ptr word that is read has an index inside (lo, hi], which the callers keep inside [0, outer - 1], and the result
    // is one of those indices: a malformed ptr gives wrong outer keys inside 1..outer (the import is refused by the verdict anyway),
    // not a read outside the caller's arrays.  lo > hi (a decreasing ptr) reads nothing.
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo + 1) >> 1);
        if ((int64_t)ptr[mid] - base <= p) lo = mid; else hi = mid - 1;
    }
    return lo;
}

template <typename IT>
__global__ __launch_bounds__(256) void k_in_expand(const IT* __restrict__ ptr, int64_t base, int64_t outer, int64_t nnz,
                                                   int64_t* __restrict__ out, long long* __restrict__ acc) {
    __shared__ int64_t sJ[2];
    int bad = 0;
    // the check: one thread per ptr word, grid-strided
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j <= outer; j += (int64_t)gridDim.x * 256) {
        const int64_t v = (int64_t)ptr[j];
        if (j == 0 && v != base) bad = 1;
        if (j == outer) { if (v != base + nnz) bad = 1; }
        else if ((int64_t)ptr[j + 1] < v) bad = 1;
    }
    // the expansion: one workgroup per item of IN_ITEM entries
    const int64_t nitems = outer > 0 ? (nnz + IN_ITEM - 1) / IN_ITEM : 0;
    for (int64_t item = blockIdx.x; item < nitems; item += gridDim.x) {
        const int64_t p0 = item * IN_ITEM;
        const int64_t p1 = (p0 + IN_ITEM < nnz ? p0 + IN_ITEM : nnz) - 1;           // the item's last entry
        if (threadIdx.x < 2) sJ[threadIdx.x] = in_slice_of(ptr, base, threadIdx.x == 0 ? p0 : p1, (int64_t)0, outer - 1);
        __syncthreads();
        const int64_t jhi = sJ[1];
        int64_t j = sJ[0];
        for (int64_t p = p0 + threadIdx.x; p <= p1; p += 256) {
            j = in_slice_of(ptr, base, p, j, jhi);      // (a thread's entries ascend: its last slice bounds the next search from below)
            out[p] = j + 1;
        }
        if (threadIdx.x == 0) {
            if (p0 == 0) acc[0] = sJ[0] + 1;            // the first and the last non-empty slice: the range of the outer keys
            if (p1 == nnz - 1) acc[1] = jhi + 1;
        }
        __syncthreads();
    }
    if (__syncthreads_or(bad) && threadIdx.x == 0) atomicOr(reinterpret_cast<unsigned long long*>(acc + 4), (unsigned long long)IN_BAD_PTR);
}

template <typename IT>
__global__ __launch_bounds__(256) void k_in_keys(const IT* __restrict__ a, const IT* __restrict__ b, int64_t shift, int64_t n,
                                                 int64_t* __restrict__ out_a, int64_t* __restrict__ out_b, long long* __restrict__ acc) {
    __shared__ long long sM[4][4];
    __shared__ unsigned int sZ;
    long long m[4] = {INT64_MAX, INT64_MIN, INT64_MAX, INT64_MIN};
    unsigned int z = 0;
    if (threadIdx.x == 0) sZ = 0u;
#pragma unroll 4
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        if (a != nullptr) {
            const long long x = (long long)((unsigned long long)(long long)a[i] + (unsigned long long)shift);
            if (out_a != nullptr) out_a[i] = x;
            m[0] = x < m[0] ? x : m[0]; m[1] = x > m[1] ? x : m[1];
            if (x == 0) z |= (unsigned int)IN_ZERO_A;
        }
        const long long y = (long long)((unsigned long long)(long long)b[i] + (unsigned long long)shift);
        if (out_b != nullptr) out_b[i] = y;
        m[2] = y < m[2] ? y : m[2]; m[3] = y > m[3] ? y : m[3];
        if (y == 0) z |= (unsigned int)IN_ZERO_B;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int q = 0; q < 4; ++q) { const long long t = __shfl_xor(m[q], o, 64); m[q] = (q & 1) ? (t > m[q] ? t : m[q]) : (t < m[q] ? t : m[q]); }
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) for (int q = 0; q < 4; ++q) sM[wv][q] = m[q];
    if (z) atomicOr(&sZ, z);
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) for (int q = 0; q < 4; ++q) m[q] = (q & 1) ? (sM[w][q] > m[q] ? sM[w][q] : m[q]) : (sM[w][q] < m[q] ? sM[w][q] : m[q]);
        if (a != nullptr) { atomicMin(acc + 0, m[0]); atomicMax(acc + 1, m[1]); }
        atomicMin(acc + 2, m[2]); atomicMax(acc + 3, m[3]);
        if (sZ) atomicOr(reinterpret_cast<unsigned long long*>(acc + 4), (unsigned long long)sZ);
    }
}

__global__ void k_in_publish(const long long* __restrict__ acc, unsigned long long* __restrict__ pinned, unsigned long long seq) {
    if (threadIdx.x != 0) return;
    for (int q = 0; q < 5; ++q) __hip_atomic_store(pinned + q, (unsigned long long)acc[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    publish_seq(pinned + 5, seq);
}

hipError_t launch_in_init(long long* d_acc, hipStream_t stream) {
    hipLaunchKernelGGL(k_in_init, dim3(1), dim3(64), 0, stream, d_acc);
    return hipGetLastError();
}

hipError_t launch_in_expand(const void* d_ptr, int32_t index_bits, int64_t base, int64_t outer, int64_t nnz, int64_t* out, long long* d_acc,
                            hipStream_t stream) {
    if (d_ptr == nullptr || outer < 0 || nnz < 0 || (nnz > 0 && out == nullptr)) return hipErrorInvalidValue;
    const int64_t nitems = outer > 0 ? (nnz + IN_ITEM - 1) / IN_ITEM : 0;
    const unsigned blocks = (unsigned)std::min<int64_t>(std::max<int64_t>(std::max<int64_t>(nitems, (outer + 1024) / 1024), 1), 8192);
    if (index_bits == 32)
        hipLaunchKernelGGL(k_in_expand<int32_t>, dim3(blocks), dim3(256), 0, stream, static_cast<const int32_t*>(d_ptr), base, outer, nnz, out, d_acc);
    else
        hipLaunchKernelGGL(k_in_expand<int64_t>, dim3(blocks), dim3(256), 0, stream, static_cast<const int64_t*>(d_ptr), base, outer, nnz, out, d_acc);
    return hipGetLastError();
}

hipError_t launch_in_keys(const void* d_a, const void* d_b, int32_t index_bits, int64_t base, int64_t n, int64_t* out_a, int64_t* out_b,
                          long long* d_acc, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    if (d_b == nullptr) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)std::min<int64_t>((n + 2047) / 2048, 2048);
    const int64_t shift = 1 - base;
    if (index_bits == 32)
        hipLaunchKernelGGL(k_in_keys<int32_t>, dim3(blocks), dim3(256), 0, stream, static_cast<const int32_t*>(d_a), static_cast<const int32_t*>(d_b),
                           shift, n, out_a, out_b, d_acc);
    else
        hipLaunchKernelGGL(k_in_keys<int64_t>, dim3(blocks), dim3(256), 0, stream, static_cast<const int64_t*>(d_a), static_cast<const int64_t*>(d_b),
                           shift, n, out_a, out_b, d_acc);
    return hipGetLastError();
}

hipError_t launch_in_publish(const long long* d_acc, unsigned long long* pinned, unsigned long long seq, hipStream_t stream) {
    hipLaunchKernelGGL(k_in_publish, dim3(1), dim3(64), 0, stream, d_acc, pinned, seq);
    return hipGetLastError();
}

}  // namespace dsa
