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
constexpr size_t PAIR_SORT_GHIST_BYTES = 8 * 256 * 4 + 64;      // ghist: 256 digit totals for each of the up to 8 passes of a run (+ 64 spare)

// Cuts 256-byte-aligned arrays off one block, front to back.  From a null base it hands out null pointers and only counts, so ONE
// layout function gives both the size of a block (bytes() after a run from nullptr) and its arrays (a run from the block).
struct Carver {
    char* base; size_t used = 0;
    explicit Carver(void* b) : base(static_cast<char*>(b)) {}
    template <typename T> T* take(size_t bytes) {
        T* p = base != nullptr ? reinterpret_cast<T*>(base + used) : nullptr;
        used += (bytes + 255) & ~(size_t)255;
        return p;
    }
    size_t bytes() const { return used; }
};

struct PairSort { uint64_t* comp[2]; double* pay[2]; uint32_t* hist; uint32_t* ghist; };
static inline PairSort pair_sort_layout(Carver& c, int64_t n) {
    const size_t nblocks = (size_t)((n + PAIR_SORT_TILE - 1) / PAIR_SORT_TILE);
    PairSort w;
    for (int b = 0; b < 2; ++b) w.comp[b] = c.take<uint64_t>((size_t)n * 8);
    for (int b = 0; b < 2; ++b) w.pay[b] = c.take<double>((size_t)n * 8);
    w.hist = c.take<uint32_t>(256 * nblocks * 4);
    w.ghist = c.take<uint32_t>(PAIR_SORT_GHIST_BYTES);
    return w;
}
static inline size_t pair_sort_bytes(int64_t n) { Carver c(nullptr); pair_sort_layout(c, n); return c.bytes(); }
static inline PairSort pair_sort_carve(void* base, int64_t n) { Carver c(base); return pair_sort_layout(c, n); }
hipError_t launch_pair_sort(const int64_t* d_part, const int64_t* d_key, int64_t n, int64_t pmin, int pbits, int64_t kmin, int kbits,
                            const PairSort& w, uint32_t* idx, int64_t* k2, int64_t* p2, hipStream_t stream);

}  // namespace dsa
