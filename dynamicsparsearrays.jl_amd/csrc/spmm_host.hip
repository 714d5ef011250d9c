// csrc/spmm_host.hip — host side of the dense multi-vector product (dsa_mat_spmm_dense[_dev]): argument checks, the orientation that
// is walked, the zeroing of Y, the launch, and the staging of operands in host memory.  Host-only unit: the kernel is in spmm.hip.
#include "host.h"
#include "spmm.h"

namespace dsa {
namespace host {

// Y = A X (transpose = 0: the rowmajor orientation, whose partitions are the rows of Y) or A' X (colmajor), enqueued on `s`.
// X: nx x k, Y: ny x k, row-major with leading dimensions ldx, ldy >= k; columns k..ldy-1 of Y are not written.
void spmm_dev(dsa_mat* h, int32_t transpose, const double* d_x, int64_t nx, int64_t k, int64_t ldx, double* d_y, int64_t ny, int64_t ldy,
              hipStream_t s) {
    if (!h->has_major) fail(DSA_EMODE, "matrix is in fill mode");
    if (k < 1) fail(DSA_EARG, "k must be at least 1");
    if (ldx < k || ldy < k) fail(DSA_EARG, "leading dimension smaller than k");
    if (nx < 0 || ny < 0) fail(DSA_EARG, "negative length");
    if ((nx > 0 && !d_x) || (ny > 0 && !d_y)) fail(DSA_EARG, "operand is NULL");
    if (ny == 0) return;
    // rows without a partition (and every row when no cell can contribute) are +0.0; the padding columns keep what they hold
    if (ldy == k) HIPCHK(hipMemsetAsync(d_y, 0, (size_t)ny * (size_t)k * sizeof(double), s));
    else HIPCHK(hipMemset2DAsync(d_y, (size_t)ldy * sizeof(double), 0, (size_t)k * sizeof(double), (size_t)ny, s));
    if (nx == 0) return;
    Pma& P = transpose ? h->col : h->row;
    // the slot stream goes around the cache when X does not fit an XCD's 4 MB L2 beside it (the rule of SPMV_PLAIN_STREAM)
    const bool nt = nx * k * (int64_t)sizeof(double) > (3 << 20);
    LAUNCH("spmm", launch_spmm(P.view(), d_x, nx, k, ldx, d_y, ny, ldy, nt, s));
}

// the same with X and Y in host memory: packed device staging (leading dimension k), one stream sync at the end
void spmm_host(dsa_mat* h, int32_t transpose, const double* x, int64_t nx, int64_t k, int64_t ldx, double* y, int64_t ny, int64_t ldy) {
    mat_flush(h);
    if (!h->has_major) fail(DSA_EMODE, "matrix is in fill mode");
    if (k < 1) fail(DSA_EARG, "k must be at least 1");
    if (ldx < k || ldy < k) fail(DSA_EARG, "leading dimension smaller than k");
    if (nx < 0 || ny < 0) fail(DSA_EARG, "negative length");
    if ((nx > 0 && !x) || (ny > 0 && !y)) fail(DSA_EARG, "operand is NULL");
    Pma& P = transpose ? h->col : h->row;
    DevStaging b(P.stream);
    const size_t row = (size_t)k * sizeof(double);
    if (nx > 0) b.upload_rows(0, x, (size_t)ldx * sizeof(double), row, (size_t)nx);
    if (ny > 0) {
        spmm_dev(h, transpose, b.at<double>(0), nx, k, k, b.alloc<double>(1, (size_t)ny * row), ny, k, P.stream);
        b.down_rows(y, (size_t)ldy * sizeof(double), 1, row, (size_t)ny);
    }
    b.sync();
}

}  // namespace host
}  // namespace dsa
