// csrc/submatrix.h — launch wrappers of the submatrix export (submatrix.hip): the partitions of an outer key list restricted to and
// renumbered by an inner key list, as one compressed matrix.  Kept apart from dsa_dev.h for the reason compress.h is.
#pragma once
#include "dsa_dev.h"

namespace dsa {

// Two pooled scratch blocks, nothing to initialise: the KEY block (hash table of the inner list, spans and work-item prefixes of the
// outer list; sized before the first launch) and the ITEM block (kept cells and owner of every work item; sized from the item count
// the first phase hands over).
size_t submatrix_key_scratch_bytes(int64_t nouter, int64_t ninner);
size_t submatrix_item_scratch_bytes(int64_t items);

// Error bits of the three phases: 1 an outer key outside 1..dim_out, 2 tables and slots out of step, 4 an inner key outside
// 1..dim_in, 8 an inner key listed twice, 16 a cell of a selected partition whose stored inner key lies outside 1..dim_in.

// Phase 1 (k_sub_hash, k_key_spans of export_dev.h, k_sub_scan_items): fills the hash table of the inner list, looks the outer keys up and cuts
// their spans into 2048-slot work items; hands {error bits, work items} and then `seq` to pinned3.
hipError_t launch_submatrix_keys(const SlotView& V, const int64_t* d_outer, int64_t nouter, int64_t dim_out, const int64_t* d_inner,
                                 int64_t ninner, int64_t dim_in, void* key_scratch, unsigned long long* pinned3, unsigned long long seq,
                                 hipStream_t stream);
// Phase 2 (k_sub_count, k_sub_scan_cells) on the key block phase 1 left: counts the kept cells of every work item, writes
// ptr[nouter + 1] (index_bits 32 | 64, ptr[j] = base + kept cells of the slices in front of j) and hands {error bits, kept cells in
// all} and then `seq` to pinned3.  items >= 0.
hipError_t launch_submatrix_count(const SlotView& V, int64_t nouter, int64_t ninner, int64_t items, int64_t dim_in, int32_t index_bits,
                                  int64_t base, void* d_ptr, void* key_scratch, void* item_scratch, unsigned long long* pinned3,
                                  unsigned long long seq, hipStream_t stream);
// Phase 3 (k_sub_emit) on both blocks: idx / vals[total]; {error bits} and then `seq` go to pinned2.  items > 0, total > 0.
hipError_t launch_submatrix_emit(const SlotView& V, int64_t nouter, int64_t ninner, int64_t items, int64_t total, int32_t index_bits,
                                 int64_t base, void* d_idx, double* d_vals, void* key_scratch, void* item_scratch,
                                 unsigned long long* pinned2, unsigned long long seq, hipStream_t stream);

}  // namespace dsa
