// csrc/selprod_host.hip — host side of the selected-key product (dsa_mat_spmm_selected[_dev]): argument checks, the orientation that
// is walked, the launch, and the staging of keys and operands in host memory.  Host-only unit: the kernel is in selprod.hip.
// Read-only and stream-ordered: no epoch moves, no scratch, no hand-over, no host wait in the device form.
#include "host.h"
#include "selprod.h"

#include <climits>

namespace dsa {
namespace host {

namespace {

// what both forms check before anything is enqueued (sel, x, y: host or device addresses, only compared with NULL)
void selprod_check(dsa_mat* h, const void* sel, int64_t nsel, const void* x, int64_t nx, int64_t k, int64_t ldx, const void* y, int64_t ldy) {
    if (h->fillmode || !h->has_major) fail(DSA_EMODE, "matrix is in fill mode");
    if (k < 1) fail(DSA_EARG, "k must be at least 1");
    if (ldx < k || ldy < k) fail(DSA_EARG, "leading dimension smaller than k");
    if (nx < 0 || nsel < 0) fail(DSA_EARG, "negative length");
    if (nsel > INT32_MAX) fail(DSA_EARG, "nsel must lie in 0 .. 2^31 - 1");
    if ((nsel > 0 && (!sel || !y)) || (nx > 0 && !x)) fail(DSA_EARG, "operand is NULL");
}

}  // namespace

// Y[j] = (partition sel[j] of the rowmajor orientation (transpose = 0: Y = A[sel, :] X) or of colmajor (Y = A[:, sel]' X)) X, enqueued
// on `s`.  X: nx x k, Y: nsel x k, row-major with leading dimensions ldx, ldy >= k; columns k..ldy-1 of Y are not written.
void selprod_dev(dsa_mat* h, int32_t transpose, const int64_t* d_sel, int64_t nsel, const double* d_x, int64_t nx, int64_t k, int64_t ldx,
                 double* d_y, int64_t ldy, hipStream_t s) {
    selprod_check(h, d_sel, nsel, d_x, nx, k, ldx, d_y, ldy);
    if (nsel == 0) return;
    Pma& P = transpose ? h->col : h->row;
    // the slot stream goes around the cache when X does not fit an XCD's 4 MB L2 beside it (the rule of spmm_dev)
    const bool nt = nx * k * (int64_t)sizeof(double) > (3 << 20);
    LAUNCH("selected product", launch_selprod(P.view(), d_sel, nsel, d_x, nx, k, ldx, d_y, ldy, nt, s));
}

// the same with the keys, X and Y in host memory: packed device staging (leading dimension k), one stream sync at the end
void selprod_host(dsa_mat* h, int32_t transpose, const int64_t* sel, int64_t nsel, const double* x, int64_t nx, int64_t k, int64_t ldx,
                  double* y, int64_t ldy) {
    mat_flush(h);
    selprod_check(h, sel, nsel, x, nx, k, ldx, y, ldy);
    for (int64_t j = 0; j < nsel; ++j)
        if (sel[j] < 1) fail(DSA_EARG, "a selected key is smaller than 1 (keys are 1-based)");
    if (nsel == 0) return;
    Pma& P = transpose ? h->col : h->row;
    DevStaging b(P.stream);
    const size_t row = (size_t)k * sizeof(double);
    const int64_t* d_sel = b.upload<int64_t>(0, sel, (size_t)nsel * sizeof(int64_t));
    if (nx > 0) b.upload_rows(1, x, (size_t)ldx * sizeof(double), row, (size_t)nx);
    selprod_dev(h, transpose, d_sel, nsel, b.at<double>(1), nx, k, k, b.alloc<double>(2, (size_t)nsel * row), k, P.stream);
    b.down_rows(y, (size_t)ldy * sizeof(double), 2, row, (size_t)nsel);
    b.sync();
}

}  // namespace host
}  // namespace dsa
