// csrc/selprod.h — launch wrapper of the selected-key product, shared by selprod.hip (the kernel) and selprod_host.hip.
#pragma once
#include "dsa_dev.h"

namespace dsa {

// Y[j, 0:k] = (live partition of P whose key is d_sel[j]) X[:, 0:k] for j in 0 .. nsel - 1, X (nx x k) and Y (nsel x k) dense and
// ROW-MAJOR with leading dimensions ldx, ldy (selprod.hip: k_selprod).  Every row of Y is stored, columns 0..k-1 only: a key without a
// live partition (and every key when nx = 0) gives +0.0.  nt: non-temporal slot loads.
hipError_t launch_selprod(const SlotView& V, const int64_t* d_sel, int64_t nsel, const double* x, int64_t nx, int64_t k, int64_t ldx,
                          double* y, int64_t ldy, bool nt, hipStream_t stream);

}  // namespace dsa
