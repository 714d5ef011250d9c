// csrc/droptol.h — launch wrappers of the in-place pruning of small entries (dropzeros! / droptol!), shared by droptol.hip (the
// kernels) and droptol_host.hip.
#pragma once
#include "dsa_dev.h"

namespace dsa {

// device scratch of one droptol of an orientation with `capacity` slots: the scale scratch (bounds word, per-span carry), one
// 4-byte counter per span, and one drop mask per occupancy word (capacity / 8 bytes)
size_t droptol_scratch_bytes(int64_t capacity);

// Pass 1 (k_drop_decide, k_drop_verdict; with a threshold vector launch_scale_check of scale.h in front, on the same stream): the
// drop mask of every occupancy word — bit = an occupied non-semaphore slot whose value v has |v| <= tol, |v| <= t_key[key - 1] or
// |v| <= t_part[key of its partition - 1] (a vector that is nullptr is absent) — and their total.  Writes nothing but the scratch;
// hands {error word, count, seq} to pinned[0..2]: bit 0 a stored entry outside dim_key x dim_part (only looked for with a vector).
// pinned[3..4] belong to the check pass.
hipError_t launch_droptol_decide(const SlotView& V, double tol, const double* t_key, int64_t dim_key, const double* t_part, int64_t dim_part,
                                 bool nt, void* scratch, unsigned long long* pinned, unsigned long long seq, hipStream_t stream);
// Pass 2 (k_drop_mark): occ[w] &= ~mask[w] on the scratch pass 1 left.  Keys, values, semaphores and tables are never written.
hipError_t launch_droptol_mark(uint64_t* occ, int64_t capacity, const void* scratch, hipStream_t stream);

}  // namespace dsa
