// csrc/compress.h — launch wrapper of the compressed export (compress.hip).  Kept apart from dsa_dev.h, whose hash keys the committed
// PMC summaries of the SpMV and rebalance kernels (bench.py: kernel_source_sha).
#pragma once
#include "dsa_dev.h"

namespace dsa {

// ptr[dim_out + 1], idx / vals[nnz] with index_bits 32 | 64 and index base `base`; scratch of compress_scratch_bytes(capacity) bytes
// (pooled, nothing to initialise); the last kernel writes {error bits: 1 an entry outside size(m), 2 slots and tables disagree} and then
// `seq` to out2_pinned.  Reads the slot array and the tables only.
size_t compress_scratch_bytes(int64_t capacity);
hipError_t launch_to_compressed(const SlotView& V, int64_t nparts, int64_t nnz, int64_t dim_out, int64_t dim_in, int32_t index_bits, int64_t base,
                                void* d_ptr, void* d_idx, double* d_vals, void* scratch, unsigned long long* out2_pinned,
                                unsigned long long seq, hipStream_t stream);

}  // namespace dsa
