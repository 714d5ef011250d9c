// csrc/select.h — launch wrappers of the selected export (select.hip): the partitions of a key list as one compressed matrix.  Kept
// apart from dsa_dev.h for the reason compress.h is.
#pragma once
#include "dsa_dev.h"

namespace dsa {

// scratch of a selection of nsel keys (pooled, nothing to initialise)
size_t select_scratch_bytes(int64_t nsel);

// Phase 1 (k_key_spans of export_dev.h, k_sel_scan): looks the keys up, writes ptr[nsel + 1] (index_bits 32 | 64, ptr[j] = base + cells of the
// selections in front of j) and hands {error bits, cells in all, work items of the emit} and then `seq` to pinned4.  Error bits:
// 1 a selected key outside 1..dim_out, 2 tables and slots out of step.
hipError_t launch_select_count(const SlotView& V, const int64_t* d_sel, int64_t nsel, int64_t dim_out, int32_t index_bits, int64_t base,
                               void* d_ptr, void* scratch, unsigned long long* pinned4, unsigned long long seq, hipStream_t stream);
// Phase 2 (k_sel_emit) on the scratch phase 1 left: idx / vals[total]; {error bits: 1 an inner key of a selected partition outside
// 1..dim_in, 2 tables and slots out of step} and then `seq` go to pinned2.  items > 0.
hipError_t launch_select_emit(const SlotView& V, int64_t nsel, int64_t items, int64_t total, int64_t dim_in, int32_t index_bits, int64_t base,
                              void* d_idx, double* d_vals, void* scratch, unsigned long long* pinned2, unsigned long long seq,
                              hipStream_t stream);

}  // namespace dsa
