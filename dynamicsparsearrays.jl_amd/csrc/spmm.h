// csrc/spmm.h — launch wrapper of the dense multi-vector product, shared by spmm.hip (the kernel) and spmm_host.hip.
#pragma once
#include "dsa_dev.h"

namespace dsa {

// Y = P X over one orientation P for k right-hand sides, X (nx x k) and Y (ny x k) dense and ROW-MAJOR with leading dimensions ldx, ldy
// (spmm.hip: k_spmm).  Writes the rows that own a partition, columns 0..k-1 only: the caller zeroes Y first.  nt: non-temporal slot loads.
hipError_t launch_spmm(const SlotView& V, const double* x, int64_t nx, int64_t k, int64_t ldx, double* y, int64_t ny, int64_t ldy, bool nt,
                       hipStream_t stream);

}  // namespace dsa
