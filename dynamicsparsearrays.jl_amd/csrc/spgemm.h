// csrc/spgemm.h — constants and launch wrappers of the batched sparse-x product (spgemm.hip): Y = A S / A' S for k sparse columns,
// both operands and the result CSC in HBM.  Kept apart from dsa_dev.h for the reason compress.h is.
#pragma once
#include "dsa_dev.h"

namespace dsa {

// A column of S whose products visit at most SPG_SMALL_MAX stored cells of A is summed in an LDS hash table of SPG_TABLE_SLOTS
// entries (8-byte key + 8-byte sum: 32 KiB, one wave per workgroup, five workgroups per CU); a longer one in a slab of ny doubles
// plus a bitmap of ny / 64 words in HBM.  At most SPG_MAX_SLABS slabs and SPG_SLAB_BYTES_MAX bytes of them exist per orientation;
// fewer slabs than long columns means their owners loop.
constexpr int64_t SPG_SMALL_MAX = 1024;
constexpr int64_t SPG_TABLE_SLOTS = 2048;
constexpr int64_t SPG_MAX_SLABS = 16;
constexpr int64_t SPG_SLAB_BYTES_MAX = 1073741824;      // 1 GiB

// error bits of the three hand-overs: 1 a touched row key outside 1..ny, 2 tables and slots out of step (or a result that
// differs from its count), 4 a probe sequence as long as the table, 8 the input contract of S violated
constexpr uint32_t SPG_ERR_BOUNDS = 1u, SPG_ERR_STEP = 2u, SPG_ERR_PROBE = 4u, SPG_ERR_INPUT = 8u;

// what the kernels are told about the four index arrays
struct SpgIndex { int32_t bits32; int32_t pad_; int64_t base; };

// scratch of a product with k columns and nnzx stored entries (pooled, nothing to initialise), and the words of one slab
size_t spgemm_scratch_bytes(int64_t k, int64_t nnzx);
int64_t spgemm_slab_words(int64_t ny);

// Phase 1 (one memset, k_spg_bound, k_spg_classify): the input contract, the span and the cell count of every stored entry of S,
// the cells each column will visit, the list of the long columns.  {error bits, long columns} and then `seq` go to pinned3.
hipError_t launch_spgemm_bound(const SlotView& V, SpgIndex ix, const void* d_xptr, const void* d_xidx, int64_t k, int64_t nnzx, void* scratch,
                               unsigned long long* pinned3, unsigned long long seq, hipStream_t stream);
// Phase 2 (k_spg_lds<count>, k_spg_slab<count> when n_large > 0, k_spg_scan) on the scratch phase 1 left: touched rows per column,
// yptr[k + 1]; {error bits, total} and then `seq` go to pinned3.  slabs: nslabs slabs, all zero, left all zero.
hipError_t launch_spgemm_count(const SlotView& V, int64_t k, int64_t nnzx, int64_t ny, int64_t n_large, uint64_t* slabs,
                               int64_t nslabs, SpgIndex ix, void* d_yptr, void* scratch, unsigned long long* pinned3, unsigned long long seq,
                               hipStream_t stream);
// Phase 3 (k_spg_lds<emit>, k_spg_slab<emit> when n_large > 0, k_spg_done): yidx / yval[total]; {error bits} and then `seq` go to
// pinned2.  total > 0.
hipError_t launch_spgemm_emit(const SlotView& V, const double* d_xval, int64_t k, int64_t nnzx, int64_t ny,
                              int64_t n_large, uint64_t* slabs, int64_t nslabs, SpgIndex ix, void* d_yidx, double* d_yval, void* scratch,
                              unsigned long long* pinned2, unsigned long long seq, hipStream_t stream);

}  // namespace dsa
