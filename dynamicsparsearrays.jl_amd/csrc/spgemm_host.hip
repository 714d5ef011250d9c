// csrc/spgemm_host.hip — host side of the batched sparse-x product (dsa_mat_spgemm_csc[_dev]): argument checks before anything is
// enqueued, the pooled scratch and the slabs of the walked orientation, the three groups of launches with their hand-overs, and the
// staging of the host form.  Host-only unit: the kernels are in spgemm.hip.  Read-only: no epoch moves, a cached SpMV plan survives.
#include "host.h"
#include "spgemm.h"

#include <algorithm>
#include <climits>

namespace dsa {
namespace host {

namespace {

struct SpgSide { Pma& P; int64_t ny; };
SpgSide spgemm_side(dsa_mat* h, int32_t transpose) {
    mat_flush(h);
    if (h->fillmode || !h->has_major) fail(DSA_EMODE, "matrix is in fill mode");
    if (transpose != 0 && transpose != 1) fail(DSA_EARG, "transpose must be 0 or 1");
    return transpose ? SpgSide{h->row, h->n} : SpgSide{h->col, h->m};
}

// the error word a kernel of the product handed over
void spgemm_verdict(const unsigned long long* word) {
    const unsigned long long err = __atomic_load_n(word, __ATOMIC_ACQUIRE);
    if (err & SPG_ERR_INPUT) fail(DSA_EARG, "S is not a valid CSC: ptr must start at the base, not decrease and end at nnzx, idx must ascend strictly within a column");
    if (err & SPG_ERR_STEP) fail(DSA_EASSERT, "sparse product: slot array and partition tables disagree");
    if (err & SPG_ERR_PROBE) fail(DSA_EASSERT, "sparse product: the hash table of a column is full");
    if (err & SPG_ERR_BOUNDS) fail(DSA_EBOUNDS, "a stored entry of a visited partition lies outside size(m)");
}

struct SpgTotals { int64_t total = 0, n_large = 0, nslabs = 0; };

// argument checks, the bound pass and the first wait (input contract, long columns), the slabs, the count pass and the second wait.
// yptr is complete when this returns; *nnz_out = entries of Y.
SpgTotals spgemm_count(const SpgSide& e, int32_t index_bits, int32_t index_base, const void* d_xptr, const void* d_xidx, const double* d_xval,
                       int64_t k, int64_t nnzx, void* d_yptr, int64_t* nnz_out) {
    Pma& P = e.P;
    if (!nnz_out) fail(DSA_EARG, "nnz_out is NULL");
    check_index_format(index_bits, index_base);
    if (k < 0 || k > INT32_MAX) fail(DSA_EARG, "k must lie in 0 .. 2^31 - 1");
    if (nnzx < 0 || nnzx > INT32_MAX) fail(DSA_EARG, "nnzx must lie in 0 .. 2^31 - 1");
    if (!d_xptr || !d_yptr || (nnzx > 0 && (!d_xidx || !d_xval))) fail(DSA_EARG, "an array of S or yptr is NULL");
    if (index_bits == 32 && e.ny > INT32_MAX) fail(DSA_EARG, "the rows of Y do not fit 32-bit indices");
    *nnz_out = 0;
    const SpgIndex ix{index_bits == 32 ? 1 : 0, 0, index_base};
    ExportArea& A = P.spg;
    // pinned {error word, long columns, sequence number} of the bound pass, {error word, total, sequence number} of the count and
    // {error word, sequence number} of the emit
    A.ensure(P.stream, spgemm_scratch_bytes(k, nnzx), 8);
    unsigned long long seq = A.next();
    LAUNCH("sparse product (bound)", launch_spgemm_bound(P.view(), ix, d_xptr, d_xidx, k, nnzx, A.scratch, A.pin, seq, P.stream));
    wait_handover(P, A.pin + 2, seq, "sparse product (bound)");
    spgemm_verdict(A.pin);
    SpgTotals t;
    t.n_large = (int64_t)A.pin[1];
    if (t.n_large > 0) {
        const int64_t slab_bytes = spgemm_slab_words(e.ny) * 8;
        if (e.ny > SPG_SLAB_BYTES_MAX / 8 || slab_bytes > SPG_SLAB_BYTES_MAX)
            fail(DSA_EARG, "a column of S visits more than SPG_SMALL_MAX = " + std::to_string(SPG_SMALL_MAX) + " stored cells and its slab of size(m) doubles exceeds SPG_SLAB_BYTES_MAX = " +
                               std::to_string(SPG_SLAB_BYTES_MAX) + " bytes");
        t.nslabs = std::min<int64_t>({t.n_large, SPG_MAX_SLABS, SPG_SLAB_BYTES_MAX / slab_bytes});
        ExportArea& S = P.spgs;
        const size_t need = (size_t)t.nslabs * (size_t)slab_bytes;
        if (S.bytes < need) {
            S.ensure(P.stream, need, 1);
            HIPCHK(hipMemsetAsync(S.scratch, 0, S.bytes, P.stream));      // the zero invariant starts here
        }
    }
    seq = A.next();
    LAUNCH("sparse product (count)", launch_spgemm_count(P.view(), k, nnzx, e.ny, t.n_large, static_cast<uint64_t*>(P.spgs.scratch), t.nslabs,
                                                         ix, d_yptr, A.scratch, A.pin + 3, seq, P.stream));
    wait_handover(P, A.pin + 5, seq, "sparse product (count)");
    spgemm_verdict(A.pin + 3);
    t.total = (int64_t)A.pin[4];
    *nnz_out = t.total;
    if (index_bits == 32 && t.total + index_base > INT32_MAX) fail(DSA_EARG, "the entries of Y do not fit 32-bit indices");
    return t;
}

// the emit on the scratch spgemm_count left, and the third wait
void spgemm_emit(const SpgSide& e, const SpgTotals& t, int32_t index_bits, int32_t index_base, const double* d_xval, int64_t k, int64_t nnzx,
                 void* d_yidx, double* d_yval) {
    if (t.total <= 0) return;
    Pma& P = e.P;
    ExportArea& A = P.spg;
    const SpgIndex ix{index_bits == 32 ? 1 : 0, 0, index_base};
    const unsigned long long seq = A.next();
    LAUNCH("sparse product (emit)", launch_spgemm_emit(P.view(), d_xval, k, nnzx, e.ny, t.n_large, static_cast<uint64_t*>(P.spgs.scratch),
                                                       t.nslabs, ix, d_yidx, d_yval, A.scratch, A.pin + 6, seq, P.stream));
    wait_handover(P, A.pin + 7, seq, "sparse product (emit)");
    spgemm_verdict(A.pin + 6);
}

}  // namespace

void spgemm_csc_dev(dsa_mat* h, int32_t transpose, int32_t index_bits, int32_t index_base, const void* d_xptr, const void* d_xidx,
                    const double* d_xval, int64_t k, int64_t nnzx, void* d_yptr, void* d_yidx, double* d_yval, int64_t cap, int64_t* nnz_out) {
    if (cap < 0) fail(DSA_EARG, "negative capacity");
    if (cap > 0 && (!d_yidx || !d_yval)) fail(DSA_EARG, "output pointer is NULL");
    const SpgSide e = spgemm_side(h, transpose);
    const SpgTotals t = spgemm_count(e, index_bits, index_base, d_xptr, d_xidx, d_xval, k, nnzx, d_yptr, nnz_out);
    if (cap < t.total) fail(DSA_ECAP, "output buffers too small");
    spgemm_emit(e, t, index_bits, index_base, d_xval, k, nnzx, d_yidx, d_yval);
}

void spgemm_csc_host(dsa_mat* h, int32_t transpose, int32_t index_base, const int64_t* xptr, const int64_t* xidx, const double* xval, int64_t k,
                     int64_t* yptr, int64_t* yidx, double* yval, int64_t cap, int64_t* nnz_out) {
    if (cap < 0) fail(DSA_EARG, "negative capacity");
    if (!xptr || !yptr || !nnz_out) fail(DSA_EARG, "xptr, yptr or nnz_out is NULL");
    if (cap > 0 && (!yidx || !yval)) fail(DSA_EARG, "output pointer is NULL");
    if (k < 0 || k > INT32_MAX) fail(DSA_EARG, "k must lie in 0 .. 2^31 - 1");
    if (index_base != 0 && index_base != 1) fail(DSA_EARG, "index_base must be 0 or 1");
    const int64_t nnzx = xptr[k] - index_base;
    if (nnzx < 0 || nnzx > INT32_MAX) fail(DSA_EARG, "xptr[k] - base must lie in 0 .. 2^31 - 1");
    if (nnzx > 0 && (!xidx || !xval)) fail(DSA_EARG, "xidx or xval is NULL");
    const SpgSide e = spgemm_side(h, transpose);
    Pma& S = e.P;
    DevStaging b(S.stream);
    // block 0: xptr, then xidx; block 1: xval; block 2: yptr; block 3: yidx, then yval
    const size_t pb = (size_t)(k + 1) * sizeof(int64_t), xb = (size_t)nnzx * sizeof(int64_t);
    int64_t* d_xptr = b.alloc<int64_t>(0, pb + std::max<size_t>(xb, 8));
    int64_t* d_xidx = d_xptr + k + 1;
    double* d_xval = b.alloc<double>(1, std::max<size_t>(xb, 8));
    b.alloc(2, pb);
    b.up(d_xptr, xptr, pb);
    if (nnzx > 0) {
        b.up(d_xidx, xidx, xb);
        b.up(d_xval, xval, xb);
    }
    const SpgTotals t = spgemm_count(e, 64, index_base, d_xptr, d_xidx, d_xval, k, nnzx, b.p[2], nnz_out);
    b.down(yptr, b.p[2], pb);
    if (cap < t.total) {
        b.sync();      // yptr is the caller's to read with DSA_ECAP
        fail(DSA_ECAP, "output buffers too small");
    }
    if (t.total > 0) {
        const size_t cb = (size_t)t.total * sizeof(int64_t);
        int64_t* d_yidx = b.alloc<int64_t>(3, 2 * cb);
        double* d_yval = reinterpret_cast<double*>(d_yidx + t.total);
        spgemm_emit(e, t, 64, index_base, d_xval, k, nnzx, d_yidx, d_yval);
        b.down(yidx, d_yidx, cb);
        b.down(yval, d_yval, cb);
    }
    b.sync();
}

}  // namespace host
}  // namespace dsa
