// csrc/ingest.h — launch wrappers of the device-side import (ingest.hip).  Kept apart from dsa_dev.h like compress.h and select.h.
#pragma once
#include "dsa_dev.h"

namespace dsa {

// entries per work item of k_in_expand: the expansion is cut by ENTRIES, a slice of any length is shared by as many items as it spans
constexpr int64_t IN_ITEM = 2048;

// the five running words of an import in HBM (k_minmax_acc's layout) and what the last launch hands to pinned memory behind them:
//   [0] a min  [1] a max  [2] b min  [3] b max  [4] flags  [5] sequence number (pinned copy only, written last)
// a = the outer keys of a compressed input / the row keys of a COO one, b = the inner keys / the column keys
constexpr int IN_WORDS = 8;
enum : unsigned long long { IN_ZERO_A = 1, IN_ZERO_B = 2, IN_BAD_PTR = 4 };

// acc <- {INT64_MAX, INT64_MIN, INT64_MAX, INT64_MIN, 0}
hipError_t launch_in_init(long long* d_acc, hipStream_t stream);
// ptr (outer + 1 words of index_bits, offset by base) -> out[p] = 1-based outer key of entry p, p < nnz; checks ptr[0] == base,
// ptr[outer] == base + nnz and that no step decreases (IN_BAD_PTR); acc[0..1] = outer key of the first / the last entry
hipError_t launch_in_expand(const void* d_ptr, int32_t index_bits, int64_t base, int64_t outer, int64_t nnz, int64_t* out, long long* d_acc,
                            hipStream_t stream);
// key = index + 1 - base of n indices of index_bits each, for a (may be nullptr) and b; out_a / out_b == nullptr: only the folds
// (min, max, zero flag of the KEYS into acc[0..1] | IN_ZERO_A and acc[2..3] | IN_ZERO_B)
hipError_t launch_in_keys(const void* d_a, const void* d_b, int32_t index_bits, int64_t base, int64_t n, int64_t* out_a, int64_t* out_b,
                          long long* d_acc, hipStream_t stream);
// acc[0..4] to pinned[0..4], then seq to pinned[5]
hipError_t launch_in_publish(const long long* d_acc, unsigned long long* pinned, unsigned long long seq, hipStream_t stream);

}  // namespace dsa
