// csrc/pairsort.h — the stable radix sort of (partition, key) pairs that the builder's general path (build.hip, which defines it)
// and the batched insert (insert.hip) share: the scratch it needs and its launch wrapper.
#pragma once
#include "dsa_dev.h"

namespace dsa {

// The stable radix sort of the builder's general path on its own, for callers that order (partition, key) pairs without building
// anything (insert.hip): by key over kbits bits, then by partition over pbits bits, the input index riding along as the payload.
// Leaves, in (partition, key, input order): idx[j] = input index, k2[j] = key, p2[j] = partition (d_part == nullptr: key order, p2
// not written).  pmin / kmin: lower bounds of the values; 2^pbits / 2^kbits exceed their spreads.  n < 2^32.  Enqueues only.
constexpr int64_t PAIR_SORT_TILE = 4096;      // elements per workgroup of a radix pass (build.hip: RS_TILE)
struct PairSort { uint64_t* comp[2]; double* pay[2]; uint32_t* hist; uint32_t* ghist; };
static inline size_t pair_sort_bytes(int64_t n) {
    const size_t a8 = ((size_t)n * 8 + 255) & ~(size_t)255, nblocks = (size_t)((n + PAIR_SORT_TILE - 1) / PAIR_SORT_TILE);
    return 4 * a8 + ((256 * nblocks * 4 + 255) & ~(size_t)255) + 8 * 256 * 4 + 256;
}
static inline PairSort pair_sort_carve(void* base, int64_t n) {
    const size_t a8 = ((size_t)n * 8 + 255) & ~(size_t)255, nblocks = (size_t)((n + PAIR_SORT_TILE - 1) / PAIR_SORT_TILE);
    char* q = static_cast<char*>(base);
    PairSort w;
    w.comp[0] = reinterpret_cast<uint64_t*>(q); w.comp[1] = reinterpret_cast<uint64_t*>(q + a8);
    w.pay[0] = reinterpret_cast<double*>(q + 2 * a8); w.pay[1] = reinterpret_cast<double*>(q + 3 * a8);
    w.hist = reinterpret_cast<uint32_t*>(q + 4 * a8);
    w.ghist = reinterpret_cast<uint32_t*>(q + 4 * a8 + ((256 * nblocks * 4 + 255) & ~(size_t)255));
    return w;
}
hipError_t launch_pair_sort(const int64_t* d_part, const int64_t* d_key, int64_t n, int64_t pmin, int pbits, int64_t kmin, int kbits,
                            const PairSort& w, uint32_t* idx, int64_t* k2, int64_t* p2, hipStream_t stream);

}  // namespace dsa
