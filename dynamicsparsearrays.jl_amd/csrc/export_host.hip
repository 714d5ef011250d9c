// csrc/export_host.hip — host side of the compressed exports: the whole orientation (dsa_mat_to_compressed[_dev], kernels in
// compress.hip), the partitions of a key list (dsa_mat_select_compressed[_dev], kernels in select.hip) and those partitions
// restricted to an inner key list (dsa_mat_submatrix_compressed[_dev], kernels in submatrix.hip).  Argument checks, the
// scratch and pinned words of an orientation (ExportArea), the hand-overs and the staging of the host forms.  Host-only unit.
// Read-only: no epoch moves (a cached SpMV plan survives), nothing about an export stays on the handle between two calls.
#include "host.h"
#include "compress.h"
#include "select.h"
#include "submatrix.h"

#include <algorithm>
#include <climits>
#include <cstring>

namespace dsa {
namespace host {

void ExportArea::ensure(hipStream_t stream, size_t need, int words) {
    if (bytes < need) {
        if (scratch) { HIPCHK(hipStreamSynchronize(stream)); pool_free(scratch); scratch = nullptr; bytes = 0; }
        HIPCHK(pool_alloc(&scratch, need));
        bytes = need;
    }
    if (!pin) {
        HIPCHK(pinned_alloc(reinterpret_cast<void**>(&pin), (size_t)words * sizeof(unsigned long long)));
        std::memset(pin, 0, (size_t)words * sizeof(unsigned long long));
        seq = 0;
    }
}
void ExportArea::release() {
    pool_free(scratch);
    pinned_free(pin);
    *this = ExportArea();
}

void check_index_format(int32_t index_bits, int32_t index_base) {
    if (index_bits != 32 && index_bits != 64) fail(DSA_EARG, "index_bits must be 32 or 64");
    if (index_base != 0 && index_base != 1) fail(DSA_EARG, "index_base must be 0 or 1");
}

// the error word an export kernel handed over: bit 2 the structure contradicts itself, bit 1 something lies outside size(m)
void export_verdict(const unsigned long long* word, const char* what, const char* outside) {
    const unsigned long long err = __atomic_load_n(word, __ATOMIC_ACQUIRE);
    if (err & 2u) fail(DSA_EASSERT, std::string(what) + ": slot array and partition tables disagree");
    if (err & 1u) fail(DSA_EBOUNDS, outside);
}

namespace {

// what every export starts with: queued writes applied, not in fill mode, the orientation and its two dimensions
struct Side { Pma& P; int64_t dim_out, dim_in; };
Side export_side(dsa_mat* h, int32_t o) {
    mat_flush(h);
    if (h->fillmode || !h->has_major) fail(DSA_EMODE, "matrix is in fill mode");
    if (o != DSA_COLMAJOR && o != DSA_ROWMAJOR) fail(DSA_EARG, "orientation must be 0 or 1");
    const bool rows = o == DSA_ROWMAJOR;
    return Side{rows ? h->row : h->col, rows ? h->m : h->n, rows ? h->n : h->m};
}

// ---- the whole orientation: CSC from colmajor, CSR from rowmajor
void compress_side(const Side& e, int32_t index_bits, int32_t index_base, void* d_ptr, void* d_idx, double* d_vals, int64_t cap,
                   int64_t* nnz_out) {
    Pma& P = e.P;
    if (!nnz_out) fail(DSA_EARG, "nnz_out is NULL");
    check_index_format(index_bits, index_base);
    const int64_t parts = P.h_ctl->nb_partitions, nnz = P.h_ctl->nb_elements - parts;
    *nnz_out = nnz;
    if (index_bits == 32 && (e.dim_out > INT32_MAX || e.dim_in > INT32_MAX || nnz + index_base > INT32_MAX))
        fail(DSA_EARG, "a dimension or nnz does not fit 32-bit indices");
    if (cap < nnz) fail(DSA_ECAP, "output buffers too small");
    if (!d_ptr || (nnz > 0 && (!d_idx || !d_vals))) fail(DSA_EARG, "output pointer is NULL");
    ExportArea& A = P.cx;
    A.ensure(P.stream, compress_scratch_bytes(P.capacity()), 2);      // pinned {error word, sequence number}
    const unsigned long long seq = A.next();
    LAUNCH("compressed export", launch_to_compressed(P.view(), parts, nnz,
                                                     e.dim_out, e.dim_in, index_bits, index_base, d_ptr, d_idx, d_vals, A.scratch, A.pin, seq, P.stream));
    wait_handover(P, A.pin + 1, seq, "compressed export");
    export_verdict(A.pin, "compressed export", "a stored entry lies outside size(m)");
}

// ---- the key-list exports: what the count phase of either leaves for its emit
struct KeyTotals { int64_t total = 0, items = 0; };       // cells to deliver, 2048-slot work items

// The shape of a key-list export into device memory: count(e) completes ptr and gives the totals, DSA_ECAP if the cells do not fit,
// else emit(e, totals).
template <typename Count, typename Emit>
void keylist_dev(dsa_mat* h, int32_t o, const void* d_idx, const double* d_vals, int64_t cap, Count count, Emit emit) {
    if (cap < 0) fail(DSA_EARG, "negative capacity");
    if (cap > 0 && (!d_idx || !d_vals)) fail(DSA_EARG, "output pointer is NULL");
    const Side e = export_side(h, o);
    const KeyTotals t = count(e);
    if (cap < t.total) fail(DSA_ECAP, "output buffers too small");
    emit(e, t);
}

// The shape of a key-list export into host memory, 64-bit indices: the keys staged in one block (the outer list, then the inner list
// if there is one), count(d_outer, d_inner, d_ptr), ptr down, DSA_ECAP if the cells do not fit, else idx / vals allocated,
// emit(totals, d_idx, d_vals) and both down.
template <typename Count, typename Emit>
void keylist_host(const Side& e, const int64_t* outer, int64_t nouter, const int64_t* inner, int64_t ninner, int64_t* ptr, int64_t* idx,
                  double* vals, int64_t cap, Count count, Emit emit) {
    Pma& S = e.P;
    DevStaging b(S.stream);
    const size_t kb = (size_t)std::max<int64_t>(nouter + ninner, 1) * sizeof(int64_t), pb = (size_t)(nouter + 1) * sizeof(int64_t);
    int64_t* d_outer = b.alloc<int64_t>(0, kb);
    int64_t* d_inner = d_outer + nouter;
    b.alloc(1, pb);
    if (nouter > 0) b.up(d_outer, outer, (size_t)nouter * sizeof(int64_t));
    if (ninner > 0) b.up(d_inner, inner, (size_t)ninner * sizeof(int64_t));
    const KeyTotals t = count(d_outer, d_inner, b.p[1]);
    b.down(ptr, b.p[1], pb);
    if (cap < t.total) {
        b.sync();      // ptr is the caller's to read with DSA_ECAP
        fail(DSA_ECAP, "output buffers too small");
    }
    if (t.total > 0) {
        const size_t cb = (size_t)t.total * sizeof(int64_t);
        b.alloc(2, cb);
        emit(t, b.p[2], b.alloc<double>(3, cb));
        b.down(idx, b.p[2], cb);
        b.down(vals, b.p[3], cb);
    }
    b.sync();
}

// ---- the partitions of a key list
// argument checks, count + scan, the first wait.  ptr is complete when this returns; *nnz_out = cells selected.
KeyTotals select_count(const Side& e, int32_t index_bits, int32_t index_base, const int64_t* d_sel, int64_t nsel, void* d_ptr,
                       int64_t* nnz_out) {
    Pma& P = e.P;
    if (!nnz_out) fail(DSA_EARG, "nnz_out is NULL");
    check_index_format(index_bits, index_base);
    if (nsel < 0 || nsel > INT32_MAX) fail(DSA_EARG, "nsel must lie in 0 .. 2^31 - 1");
    if (!d_ptr || (nsel > 0 && !d_sel)) fail(DSA_EARG, "selection or ptr is NULL");
    if (index_bits == 32 && e.dim_in > INT32_MAX) fail(DSA_EARG, "the inner dimension does not fit 32-bit indices");
    *nnz_out = 0;
    ExportArea& A = P.sel;
    // pinned {error word, cells, work items, sequence number} of the count and {error word, sequence number} of the emit
    A.ensure(P.stream, select_scratch_bytes(nsel), 6);
    const unsigned long long seq = A.next();
    LAUNCH("selected export (count)", launch_select_count(P.view(), d_sel, nsel, e.dim_out, index_bits, index_base, d_ptr, A.scratch, A.pin,
                                                          seq, P.stream));
    wait_handover(P, A.pin + 3, seq, "selected export (count)");
    export_verdict(A.pin, "selected export", "a selected key lies outside size(m)");
    KeyTotals t;
    t.total = (int64_t)A.pin[1]; t.items = (int64_t)A.pin[2];
    *nnz_out = t.total;
    if (index_bits == 32 && t.total + index_base > INT32_MAX) fail(DSA_EARG, "the selected cells do not fit 32-bit indices");
    return t;
}

// the emit on the scratch select_count left, and the second wait
void select_emit(const Side& e, const KeyTotals& t, int32_t index_bits, int32_t index_base, int64_t nsel, void* d_idx, double* d_vals) {
    if (t.total <= 0) return;
    if (t.items <= 0) fail(DSA_EASSERT, "selected export: cells without a work item");
    Pma& P = e.P;
    ExportArea& A = P.sel;
    const unsigned long long seq = A.next();
    LAUNCH("selected export (emit)", launch_select_emit(P.view(), nsel, t.items, t.total, e.dim_in, index_bits,
                                                        index_base, d_idx, d_vals, A.scratch, A.pin + 4, seq, P.stream));
    wait_handover(P, A.pin + 5, seq, "selected export (emit)");
    export_verdict(A.pin + 4, "selected export", "a stored entry of a selected partition lies outside size(m)");
}

// ---- the partitions of an outer key list, restricted to and renumbered by an inner key list

// the error word a submatrix kernel handed over (submatrix.h lists the bits)
void submatrix_verdict(const unsigned long long* word) {
    const unsigned long long err = __atomic_load_n(word, __ATOMIC_ACQUIRE);
    if (err & 2u) fail(DSA_EASSERT, "submatrix export: slot array and partition tables disagree");
    if (err & 1u) fail(DSA_EBOUNDS, "an outer key lies outside size(m)");
    if (err & 4u) fail(DSA_EBOUNDS, "an inner key lies outside size(m)");
    if (err & 8u) fail(DSA_EARG, "an inner key is listed twice");
    if (err & 16u) fail(DSA_EBOUNDS, "a stored entry of a selected partition lies outside size(m)");
}

// argument checks, the key phase, the first wait (work items), the count phase, the second wait (kept cells).  ptr is complete
// when this returns; *nnz_out = cells kept.
KeyTotals submatrix_count(const Side& e, int32_t index_bits, int32_t index_base, const int64_t* d_outer, int64_t nouter,
                          const int64_t* d_inner, int64_t ninner, void* d_ptr, int64_t* nnz_out) {
    Pma& P = e.P;
    if (!nnz_out) fail(DSA_EARG, "nnz_out is NULL");
    check_index_format(index_bits, index_base);
    if (nouter < 0 || nouter > INT32_MAX) fail(DSA_EARG, "nouter must lie in 0 .. 2^31 - 1");
    if (ninner < 0 || ninner > INT32_MAX) fail(DSA_EARG, "ninner must lie in 0 .. 2^31 - 1");
    if (!d_ptr || (nouter > 0 && !d_outer) || (ninner > 0 && !d_inner)) fail(DSA_EARG, "a key list or ptr is NULL");
    *nnz_out = 0;
    ExportArea& A = P.sub;
    ExportArea& I = P.subi;
    // pinned {error word, work items, sequence number} of the key phase, {error word, kept cells, sequence number} of the count and
    // {error word, sequence number} of the emit
    A.ensure(P.stream, submatrix_key_scratch_bytes(nouter, ninner), 8);
    unsigned long long seq = A.next();
    LAUNCH("submatrix export (keys)", launch_submatrix_keys(P.view(), d_outer, nouter, e.dim_out, d_inner, ninner, e.dim_in, A.scratch, A.pin,
                                                            seq, P.stream));
    wait_handover(P, A.pin + 2, seq, "submatrix export (keys)");
    submatrix_verdict(A.pin);
    KeyTotals t;
    t.items = (int64_t)A.pin[1];
    I.ensure(P.stream, submatrix_item_scratch_bytes(t.items), 1);
    seq = A.next();
    LAUNCH("submatrix export (count)", launch_submatrix_count(P.view(), nouter, ninner, t.items, e.dim_in, index_bits,
                                                              index_base, d_ptr, A.scratch, I.scratch, A.pin + 3, seq, P.stream));
    wait_handover(P, A.pin + 5, seq, "submatrix export (count)");
    submatrix_verdict(A.pin + 3);
    t.total = (int64_t)A.pin[4];
    *nnz_out = t.total;
    if (index_bits == 32 && t.total + index_base > INT32_MAX) fail(DSA_EARG, "the kept cells do not fit 32-bit indices");
    return t;
}

// the emit on the scratch submatrix_count left, and the third wait
void submatrix_emit(const Side& e, const KeyTotals& t, int32_t index_bits, int32_t index_base, int64_t nouter, int64_t ninner, void* d_idx,
                    double* d_vals) {
    if (t.total <= 0) return;
    if (t.items <= 0) fail(DSA_EASSERT, "submatrix export: cells without a work item");
    Pma& P = e.P;
    ExportArea& A = P.sub;
    const unsigned long long seq = A.next();
    LAUNCH("submatrix export (emit)", launch_submatrix_emit(P.view(), nouter, ninner, t.items, t.total, index_bits,
                                                            index_base, d_idx, d_vals, A.scratch, P.subi.scratch, A.pin + 6, seq, P.stream));
    wait_handover(P, A.pin + 7, seq, "submatrix export (emit)");
    submatrix_verdict(A.pin + 6);
}

}  // namespace

void to_compressed_dev(dsa_mat* h, int32_t o, int32_t index_bits, int32_t index_base, void* d_ptr, void* d_idx, double* d_vals,
                       int64_t cap, int64_t* nnz_out) {
    compress_side(export_side(h, o), index_bits, index_base, d_ptr, d_idx, d_vals, cap, nnz_out);
}

void to_compressed_host(dsa_mat* h, int32_t o, int32_t index_base, int64_t* ptr, int64_t* idx, double* vals, int64_t cap,
                        int64_t* nnz_out) {
    const Side e = export_side(h, o);
    Pma& P = e.P;
    if (!ptr || !nnz_out) fail(DSA_EARG, "output pointer is NULL");
    const int64_t nnz = P.h_ctl->nb_elements - P.h_ctl->nb_partitions;
    *nnz_out = nnz;
    if (cap < nnz) fail(DSA_ECAP, "output buffers too small");
    if (nnz > 0 && (!idx || !vals)) fail(DSA_EARG, "output pointer is NULL");
    DevStaging b(P.stream);
    const size_t pb = (size_t)(e.dim_out + 1) * sizeof(int64_t), cb = (size_t)std::max<int64_t>(nnz, 1) * sizeof(int64_t);
    b.alloc(0, pb);
    b.alloc(1, cb);
    int64_t n = 0;
    compress_side(e, 64, index_base, b.p[0], b.p[1], b.alloc<double>(2, cb), nnz, &n);
    b.down(ptr, b.p[0], pb);
    if (n > 0) {
        b.down(idx, b.p[1], (size_t)n * sizeof(int64_t));
        b.down(vals, b.p[2], (size_t)n * sizeof(double));
    }
    b.sync();
}

void select_compressed_dev(dsa_mat* h, int32_t o, int32_t index_bits, int32_t index_base, const int64_t* d_sel, int64_t nsel,
                           void* d_ptr, void* d_idx, double* d_vals, int64_t cap, int64_t* nnz_out) {
    keylist_dev(h, o, d_idx, d_vals, cap,
                [&](const Side& e) { return select_count(e, index_bits, index_base, d_sel, nsel, d_ptr, nnz_out); },
                [&](const Side& e, const KeyTotals& t) { select_emit(e, t, index_bits, index_base, nsel, d_idx, d_vals); });
}

void select_compressed_host(dsa_mat* h, int32_t o, int32_t index_base, const int64_t* sel, int64_t nsel, int64_t* ptr, int64_t* idx,
                            double* vals, int64_t cap, int64_t* nnz_out) {
    if (cap < 0) fail(DSA_EARG, "negative capacity");
    if (!ptr || !nnz_out || (nsel > 0 && !sel)) fail(DSA_EARG, "selection, ptr or nnz_out is NULL");
    if (cap > 0 && (!idx || !vals)) fail(DSA_EARG, "output pointer is NULL");
    if (nsel < 0 || nsel > INT32_MAX) fail(DSA_EARG, "nsel must lie in 0 .. 2^31 - 1");
    const Side e = export_side(h, o);
    keylist_host(e, sel, nsel, nullptr, 0, ptr, idx, vals, cap,
                 [&](const int64_t* d_sel, const int64_t*, void* d_ptr) { return select_count(e, 64, index_base, d_sel, nsel, d_ptr, nnz_out); },
                 [&](const KeyTotals& t, void* d_idx, double* d_vals) { select_emit(e, t, 64, index_base, nsel, d_idx, d_vals); });
}

void submatrix_compressed_dev(dsa_mat* h, int32_t o, int32_t index_bits, int32_t index_base, const int64_t* d_outer, int64_t nouter,
                              const int64_t* d_inner, int64_t ninner, void* d_ptr, void* d_idx, double* d_vals, int64_t cap,
                              int64_t* nnz_out) {
    keylist_dev(h, o, d_idx, d_vals, cap,
                [&](const Side& e) { return submatrix_count(e, index_bits, index_base, d_outer, nouter, d_inner, ninner, d_ptr, nnz_out); },
                [&](const Side& e, const KeyTotals& t) { submatrix_emit(e, t, index_bits, index_base, nouter, ninner, d_idx, d_vals); });
}

void submatrix_compressed_host(dsa_mat* h, int32_t o, int32_t index_base, const int64_t* outer, int64_t nouter, const int64_t* inner,
                               int64_t ninner, int64_t* ptr, int64_t* idx, double* vals, int64_t cap, int64_t* nnz_out) {
    if (cap < 0) fail(DSA_EARG, "negative capacity");
    if (!ptr || !nnz_out || (nouter > 0 && !outer) || (ninner > 0 && !inner)) fail(DSA_EARG, "a key list, ptr or nnz_out is NULL");
    if (cap > 0 && (!idx || !vals)) fail(DSA_EARG, "output pointer is NULL");
    if (nouter < 0 || nouter > INT32_MAX) fail(DSA_EARG, "nouter must lie in 0 .. 2^31 - 1");
    if (ninner < 0 || ninner > INT32_MAX) fail(DSA_EARG, "ninner must lie in 0 .. 2^31 - 1");
    const Side e = export_side(h, o);
    keylist_host(e, outer, nouter, inner, ninner, ptr, idx, vals, cap,
                 [&](const int64_t* d_outer, const int64_t* d_inner, void* d_ptr) {
                     return submatrix_count(e, 64, index_base, d_outer, nouter, d_inner, ninner, d_ptr, nnz_out);
                 },
                 [&](const KeyTotals& t, void* d_idx, double* d_vals) { submatrix_emit(e, t, 64, index_base, nouter, ninner, d_idx, d_vals); });
}

}  // namespace host
}  // namespace dsa
