// csrc/seq_dev.h — what the write sequencer (sequencer.hip) and the bitmap replay of an append run (appendrun.hip) share: the
// geometry of their one workgroup, the state of a pass that works on the occupancy bitmap alone, and the primitives on that state.
// Device code only.
#pragma once
#include "wave_dev.h"
#include "find_dev.h"

namespace dsa {

constexpr int SEQ_BLOCK = 256;
constexpr int64_t SMALL_W = 8192;
constexpr int64_t RUN_MIN = 64;              // shortest append run worth a replay (detection: sequencer.hip)

// A bitmap-only pass: the occupancy words, the geometry of the array, the density bounds, the counters it keeps.  The append
// replay runs on exactly this; the sequencer's Seq adds the cells, the tables and its LDS staging.
struct SeqBits {
    uint64_t* occ;
    Ctl* ctl;
    int64_t capacity, seg, height, nb_elements;
    int64_t stat_window_slots, stat_rebalances, stat_small;
    int64_t* sRed;                 // [SEQ_BLOCK/64] block-reduce scratch
    const int64_t* lo; const int64_t* hi;   // integer density bounds per level (LDS copy of Ctl::lo / Ctl::hi)
};

// _nbcells(array, from, to), `to` excluded  src/utils.jl:48-58
static __device__ int64_t blk_count(SeqBits& S, int64_t from, int64_t to) {
    if (from >= to) return 0;
    const int64_t lo0 = from - 1, hi0 = to - 2;
    const int64_t w0 = lo0 >> 6, w1 = hi0 >> 6;
    if (w1 - w0 < 8) {                                   // tiny range: every thread counts it itself
        int64_t c = 0;
        for (int64_t w = w0; w <= w1; ++w) c += popc64(S.occ[w] & word_range_mask(w, lo0, hi0));
        return c;
    }
    int64_t c = 0;
    for (int64_t w = w0 + threadIdx.x; w <= w1; w += SEQ_BLOCK) c += popc64(S.occ[w] & word_range_mask(w, lo0, hi0));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) S.sRed[threadIdx.x >> 6] = c;
    __syncthreads();
    int64_t tot = 0;
#pragma unroll
    for (int k = 0; k < SEQ_BLOCK / 64; ++k) tot += S.sRed[k];
    return tot;
}

__device__ __forceinline__ void occ_set(SeqBits& S, int64_t pos) { S.occ[(pos - 1) >> 6] |= 1ull << ((pos - 1) & 63); }
__device__ __forceinline__ void occ_clear(SeqBits& S, int64_t pos) { S.occ[(pos - 1) >> 6] &= ~(1ull << ((pos - 1) & 63)); }

}  // namespace dsa
