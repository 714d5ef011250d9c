// csrc/scale.h — launch wrappers of the per-partition reductions and of the in-place diagonal scaling, shared by scale.hip (the
// kernels) and scale_host.hip.
#pragma once
#include "dsa_dev.h"

namespace dsa {

enum RedKind : int32_t { RED_SUM = 0, RED_ABSSUM = 1, RED_SQSUM = 2, RED_ABSMAX = 3, RED_COUNT = 4 };      // include/dsa.h: DSA_RED_*

// device scratch of one reduce / one scale of an orientation with `capacity` slots (header words + per-span records)
size_t reduce_scratch_bytes(int64_t capacity);
size_t scale_scratch_bytes(int64_t capacity);

// out[part_key(p) - 1] = reduction `kind` over the cells of partition p, for every partition that has a semaphore in the slot array
// (scale.hip: k_reduce, k_reduce_finish).  Elements of out without a partition are NOT written: the caller zeroes out first.  The last
// kernel hands {error word, seq} to pinned[0..1]: bit 0 a partition key outside 1..n_out, bit 1 a semaphore whose id is not in the tables.
hipError_t launch_reduce(const SlotView& V, int32_t kind, double* out, int64_t n_out, bool nt, void* scratch, unsigned long long* pinned,
                         unsigned long long seq, hipStream_t stream);

// The pass in front of a scale (k_scale_check, k_scale_tables, k_scale_carry): per span the partition that is open at its start, and
// the bounds word — bit 0: a cell key outside 1..dim_key or the key of a live partition outside 1..dim_part.  Writes nothing but the
// scratch; hands {error word, seq} to pinned[0..1].
hipError_t launch_scale_check(const SlotView& V, int64_t dim_key, int64_t dim_part, void* scratch, unsigned long long* pinned,
                              unsigned long long seq, hipStream_t stream);
// value = ((value * alpha) * r) * c at every occupied non-semaphore slot (k_scale), on the scratch launch_scale_check left.  f_key is
// indexed by the cell's key, f_part by its partition's key (either may be nullptr: factor absent); key_is_row: f_key is r (colmajor).
hipError_t launch_scale_apply(KeyArr keys, double* vals, const uint64_t* occ, int64_t capacity, const int64_t* part_keys, int64_t table_len,
                              double alpha, const double* f_key, int64_t dim_key, const double* f_part, int64_t dim_part, bool key_is_row,
                              bool nt, const void* scratch, hipStream_t stream);

}  // namespace dsa
