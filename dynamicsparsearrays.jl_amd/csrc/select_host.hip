// csrc/select_host.hip — host side of the selected export (dsa_mat_select_compressed[_dev]): argument checks, the scratch of an
// orientation, the two hand-overs (totals behind the count, bounds word behind the emit) and the staging of the host form.  Host-only
// unit: the kernels are in select.hip.  Read-only: no epoch moves, nothing about a selection stays on the handle between two calls.
#include "host.h"
#include "select.h"

#include <algorithm>
#include <climits>
#include <cstring>

namespace dsa {
namespace host {

namespace {

struct SelTotals { int64_t total = 0, items = 0, dim_in = 0; };

// flush, mode and argument checks, count + scan, the first wait.  ptr is complete when this returns; *nnz_out = cells selected.
SelTotals select_count(dsa_mat* h, Pma*& Pout, int32_t o, int32_t index_bits, int32_t index_base, const int64_t* d_sel, int64_t nsel,
                       void* d_ptr, int64_t* nnz_out) {
    mat_flush(h);
    if (h->fillmode || !h->has_major) fail(DSA_EMODE, "matrix is in fill mode");
    if (o != DSA_COLMAJOR && o != DSA_ROWMAJOR) fail(DSA_EARG, "orientation must be 0 or 1");
    Pma& P = o == DSA_COLMAJOR ? h->col : h->row;
    Pout = &P;
    if (!nnz_out) fail(DSA_EARG, "nnz_out is NULL");
    if (index_bits != 32 && index_bits != 64) fail(DSA_EARG, "index_bits must be 32 or 64");
    if (index_base != 0 && index_base != 1) fail(DSA_EARG, "index_base must be 0 or 1");
    if (nsel < 0 || nsel > INT32_MAX) fail(DSA_EARG, "nsel must lie in 0 .. 2^31 - 1");
    if (!d_ptr || (nsel > 0 && !d_sel)) fail(DSA_EARG, "selection or ptr is NULL");
    const int64_t dim_out = o == DSA_ROWMAJOR ? h->m : h->n, dim_in = o == DSA_ROWMAJOR ? h->n : h->m;
    if (index_bits == 32 && dim_in > INT32_MAX) fail(DSA_EARG, "the inner dimension does not fit 32-bit indices");
    *nnz_out = 0;
    const size_t need = select_scratch_bytes(nsel);
    if (P.sel_bytes < need) {
        if (P.sel_scratch) { HIPCHK(hipStreamSynchronize(P.stream)); pool_free(P.sel_scratch); P.sel_scratch = nullptr; P.sel_bytes = 0; }
        HIPCHK(pool_alloc(&P.sel_scratch, need));
        P.sel_bytes = need;
    }
    if (!P.h_sel) {
        HIPCHK(pinned_alloc(reinterpret_cast<void**>(&P.h_sel), 6 * sizeof(unsigned long long)));
        std::memset(P.h_sel, 0, 6 * sizeof(unsigned long long));
        P.sel_seq = 0;
    }
    const unsigned long long seq = ++P.sel_seq;
    const Ctl& c = *P.h_ctl;
    LAUNCH("selected export (count)", launch_select_count(P.O(), c.capacity, P.sems, P.col_keys, P.col_live, c.table_len,
                                                          c.nb_partitions == c.table_len, d_sel, nsel, dim_out, index_bits, index_base,
                                                          d_ptr, P.sel_scratch, P.h_sel, seq, P.stream));
    wait_handover(P, P.h_sel + 3, seq, "selected export (count)");
    const unsigned long long err = __atomic_load_n(P.h_sel, __ATOMIC_ACQUIRE);
    if (err & 2u) fail(DSA_EASSERT, "selected export: slot array and partition tables disagree");
    if (err & 1u) fail(DSA_EBOUNDS, "a selected key lies outside size(m)");
    SelTotals t;
    t.total = (int64_t)P.h_sel[1]; t.items = (int64_t)P.h_sel[2]; t.dim_in = dim_in;
    *nnz_out = t.total;
    if (index_bits == 32 && t.total + index_base > INT32_MAX) fail(DSA_EARG, "the selected cells do not fit 32-bit indices");
    return t;
}

// the emit on the scratch select_count left, and the second wait
void select_emit(Pma& P, const SelTotals& t, int32_t index_bits, int32_t index_base, int64_t nsel, void* d_idx, double* d_vals) {
    if (t.total <= 0) return;
    if (t.items <= 0) fail(DSA_EASSERT, "selected export: cells without a work item");
    const unsigned long long seq = ++P.sel_seq;
    LAUNCH("selected export (emit)", launch_select_emit(P.K(), P.V(), P.O(), P.capacity(), nsel, t.items, t.total, t.dim_in, index_bits,
                                                        index_base, d_idx, d_vals, P.sel_scratch, P.h_sel + 4, seq, P.stream));
    wait_handover(P, P.h_sel + 5, seq, "selected export (emit)");
    const unsigned long long err = __atomic_load_n(P.h_sel + 4, __ATOMIC_ACQUIRE);
    if (err & 2u) fail(DSA_EASSERT, "selected export: slot array and partition tables disagree");
    if (err & 1u) fail(DSA_EBOUNDS, "a stored entry of a selected partition lies outside size(m)");
}

}  // namespace

void select_compressed_dev(dsa_mat* h, int32_t o, int32_t index_bits, int32_t index_base, const int64_t* d_sel, int64_t nsel,
                           void* d_ptr, void* d_idx, double* d_vals, int64_t cap, int64_t* nnz_out) {
    if (cap < 0) fail(DSA_EARG, "negative capacity");
    if (cap > 0 && (!d_idx || !d_vals)) fail(DSA_EARG, "output pointer is NULL");
    Pma* P = nullptr;
    const SelTotals t = select_count(h, P, o, index_bits, index_base, d_sel, nsel, d_ptr, nnz_out);
    if (cap < t.total) fail(DSA_ECAP, "output buffers too small");
    select_emit(*P, t, index_bits, index_base, nsel, d_idx, d_vals);
}

void select_compressed_host(dsa_mat* h, int32_t o, int32_t index_base, const int64_t* sel, int64_t nsel, int64_t* ptr, int64_t* idx,
                            double* vals, int64_t cap, int64_t* nnz_out) {
    if (cap < 0) fail(DSA_EARG, "negative capacity");
    if (!ptr || !nnz_out || (nsel > 0 && !sel)) fail(DSA_EARG, "selection, ptr or nnz_out is NULL");
    if (cap > 0 && (!idx || !vals)) fail(DSA_EARG, "output pointer is NULL");
    if (nsel < 0 || nsel > INT32_MAX) fail(DSA_EARG, "nsel must lie in 0 .. 2^31 - 1");
    mat_flush(h);
    if (h->fillmode || !h->has_major) fail(DSA_EMODE, "matrix is in fill mode");
    if (o != DSA_COLMAJOR && o != DSA_ROWMAJOR) fail(DSA_EARG, "orientation must be 0 or 1");
    Pma& S = o == DSA_COLMAJOR ? h->col : h->row;
    struct Bufs {      // device staging; released once the stream has drained (also on an error after a launch)
        hipStream_t s; void* p[4] = {nullptr, nullptr, nullptr, nullptr};
        ~Bufs() { if (p[0] || p[1] || p[2] || p[3]) { (void)hipStreamSynchronize(s); for (void* q : p) pool_free(q); } }
    } b{S.stream};
    const size_t sb = (size_t)std::max<int64_t>(nsel, 1) * sizeof(int64_t), pb = (size_t)(nsel + 1) * sizeof(int64_t);
    HIPCHK(pool_alloc(&b.p[0], sb));
    HIPCHK(pool_alloc(&b.p[1], pb));
    if (nsel > 0) HIPCHK(hipMemcpyAsync(b.p[0], sel, (size_t)nsel * sizeof(int64_t), hipMemcpyHostToDevice, S.stream));
    Pma* P = nullptr;
    const SelTotals t = select_count(h, P, o, 64, index_base, static_cast<const int64_t*>(b.p[0]), nsel, b.p[1], nnz_out);
    HIPCHK(hipMemcpyAsync(ptr, b.p[1], pb, hipMemcpyDeviceToHost, S.stream));
    if (cap < t.total) {
        HIPCHK(hipStreamSynchronize(S.stream));      // ptr is the caller's to read with DSA_ECAP
        fail(DSA_ECAP, "output buffers too small");
    }
    if (t.total > 0) {
        const size_t cb = (size_t)t.total * sizeof(int64_t);
        HIPCHK(pool_alloc(&b.p[2], cb));
        HIPCHK(pool_alloc(&b.p[3], cb));
        select_emit(S, t, 64, index_base, nsel, b.p[2], static_cast<double*>(b.p[3]));
        HIPCHK(hipMemcpyAsync(idx, b.p[2], cb, hipMemcpyDeviceToHost, S.stream));
        HIPCHK(hipMemcpyAsync(vals, b.p[3], cb, hipMemcpyDeviceToHost, S.stream));
    }
    HIPCHK(hipStreamSynchronize(S.stream));
}

}  // namespace host
}  // namespace dsa
