// csrc/combine.h — launch wrapper of K-combine (combine.hip): the stored cells of a colmajor orientation as scaled, shifted (I, J, V)
// triples in findnz order, with the ranges of their keys.  Kept apart from dsa_dev.h like compress.h.
#pragma once
#include "dsa_dev.h"

namespace dsa {

// the pinned words of one pass: {error word, row min, row max, column min, column max, sequence number}
constexpr int CB_WORDS = 6;
// error bits: 2 slots and tables disagree, 4 a shifted key is 0 (the reserved semaphore key)
constexpr unsigned CB_ASSERT = 2u, CB_ZERO_KEY = 4u;

// The four range words are the keys BEFORE the shift (a shift keeps the order, and the host can tell whether it leaves int64), min
// and max over the stored cells, in the form the kernel accumulates them with one unsigned atomicMax each from a zeroed word:
// max as key ^ 2^63, min as the complement of that.  cb_range decodes a pair; lo > hi: no cell.
static inline void cb_range(unsigned long long wmin, unsigned long long wmax, int64_t* lo, int64_t* hi) {
    *lo = (int64_t)(~wmin ^ 0x8000000000000000ull);
    *hi = (int64_t)(wmax ^ 0x8000000000000000ull);
}

// I / J / V [nnz] receive (row key + row_off, key of the owning partition + col_off, scale * value) of every stored cell in slot order;
// scratch of combine_scratch_bytes(capacity) bytes (pooled, nothing to initialise); the last kernel writes the CB_WORDS words to
// `pinned`, `seq` last.  Reads the slot array and the tables only.  Three launches and one memset, whatever nnz and the table length.
size_t combine_scratch_bytes(int64_t capacity);
hipError_t launch_combine(const SlotView& V, int64_t nparts, int64_t nnz, int64_t* d_I, int64_t* d_J, double* d_V, double scale,
                          int64_t row_off, int64_t col_off, void* scratch, unsigned long long* pinned, unsigned long long seq,
                          hipStream_t stream);

}  // namespace dsa
