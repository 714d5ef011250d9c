// csrc/scale_host.hip — host side of the per-partition reductions (dsa_mat_reduce[_dev]) and of the in-place diagonal scaling
// (dsa_mat_scale[_dev]): argument checks, the orientation that is walked, the scratch and pinned words (Pma::sc), the hand-overs of
// the bounds word and the staging of a reduce into host memory.  Host-only unit: the kernels are in scale.hip.
// Reduce is read-only: no epoch moves, a cached SpMV plan survives.  Scale changes values only — no slot moves, no layout epoch —
// and the entry point (mutate_host.hip) bumps the content epoch between scale_prepare and scale_apply.
#include "host.h"
#include "scale.h"

#include <algorithm>

namespace dsa {
namespace host {

// the slot stream goes around the cache when it does not fit an XCD's 4 MB L2 beside the vectors (the rule of spmm_dev)
bool stream_nt(const Pma& P, int64_t vector_bytes) {
    return P.capacity() * (int64_t)(P.kb() + sizeof(double)) + vector_bytes > (3 << 20);
}

// what both forms of a scale, and the host form of a droptol, check before anything is staged or launched (r, c: host or device addresses)
void scale_check_args(dsa_mat* h, const double* r, int64_t nr, const double* c, int64_t nc) {
    if (h->fillmode || !h->has_major) fail(DSA_EMODE, "matrix is in fill mode");
    if (r && nr != h->m) fail(DSA_EARG, "nr must equal the number of rows");
    if (c && nc != h->n) fail(DSA_EARG, "nc must equal the number of columns");
}

// out[key - 1] = reduction over the stored cells of partition `key` of the orientation, enqueued on its stream; waits for the bounds word
void reduce_dev(dsa_mat* h, int32_t orientation, int32_t kind, double* d_out, int64_t n_out) {
    mat_flush(h);
    if (h->fillmode || !h->has_major) fail(DSA_EMODE, "matrix is in fill mode");
    if (orientation != DSA_COLMAJOR && orientation != DSA_ROWMAJOR) fail(DSA_EARG, "orientation must be 0 or 1");
    if (kind < DSA_RED_SUM || kind > DSA_RED_COUNT) fail(DSA_EARG, "kind must be one of DSA_RED_*");
    const bool rows = orientation == DSA_ROWMAJOR;
    if (n_out != (rows ? h->m : h->n)) fail(DSA_EARG, rows ? "n_out must equal the number of rows" : "n_out must equal the number of columns");
    if (n_out > 0 && !d_out) fail(DSA_EARG, "output is NULL");
    Pma& P = rows ? h->row : h->col;
    // keys without a partition are +0.0: the kernels store the others once
    if (n_out > 0) HIPCHK(hipMemsetAsync(d_out, 0, (size_t)n_out * sizeof(double), P.stream));
    if (P.capacity() <= 0) return;                // no slot array: nothing is stored
    ExportArea& A = P.sc;
    A.ensure(P.stream, std::max(reduce_scratch_bytes(P.capacity()), scale_scratch_bytes(P.capacity())), 2);      // pinned {error word, sequence number}
    const unsigned long long seq = A.next();
    LAUNCH("reduce", launch_reduce(P.view(), kind, d_out, n_out,
                                   stream_nt(P, n_out * (int64_t)sizeof(double)), A.scratch, A.pin, seq, P.stream));
    wait_handover(P, A.pin + 1, seq, "reduce");
    export_verdict(A.pin, "reduce", rows ? "a stored row lies outside size(m)" : "a stored column lies outside size(m)");
}

void reduce_host(dsa_mat* h, int32_t orientation, int32_t kind, double* out, int64_t n_out) {
    mat_flush(h);
    if (h->fillmode || !h->has_major) fail(DSA_EMODE, "matrix is in fill mode");
    if (orientation != DSA_COLMAJOR && orientation != DSA_ROWMAJOR) fail(DSA_EARG, "orientation must be 0 or 1");
    if (n_out < 0 || (n_out > 0 && !out)) fail(DSA_EARG, "output is NULL");
    Pma& P = orientation == DSA_ROWMAJOR ? h->row : h->col;
    DevStaging b(P.stream);
    reduce_dev(h, orientation, kind, b.alloc<double>(0, (size_t)std::max<int64_t>(n_out, 1) * sizeof(double)), n_out);
    if (n_out > 0) b.down(out, b.p[0], (size_t)n_out * sizeof(double));
    b.sync();
}

// Everything of a scale in front of the first write: queued writes applied, arguments checked, and the pass over both orientations
// that finds the carry of every span and checks every stored entry against size(m).  Throws DSA_EBOUNDS with nothing modified.
void scale_prepare(dsa_mat* h, const double* d_r, int64_t nr, const double* d_c, int64_t nc) {
    mat_flush(h);
    scale_check_args(h, d_r, nr, d_c, nc);
    unsigned long long seq[2] = {0, 0};
    Pma* const side[2] = {&h->col, &h->row};
    if (h->col.capacity() <= 0 || h->row.capacity() <= 0) return;      // no slot array: nothing is stored
    for (int o = 0; o < 2; ++o) {
        Pma& P = *side[o];
        ExportArea& A = P.sc;
        A.ensure(P.stream, std::max(reduce_scratch_bytes(P.capacity()), scale_scratch_bytes(P.capacity())), 2);
        seq[o] = A.next();
        // colmajor: keys are rows, partitions columns; rowmajor: the other way round
        LAUNCH("scale (check)", launch_scale_check(P.view(), o == 0 ? h->m : h->n,
                                                   o == 0 ? h->n : h->m, A.scratch, A.pin, seq[o], P.stream));
    }
    for (int o = 0; o < 2; ++o) wait_handover(*side[o], side[o]->sc.pin + 1, seq[o], "scale (check)");
    for (int o = 0; o < 2; ++o) export_verdict(side[o]->sc.pin, "scale", "a stored entry lies outside size(m)");
}

// the writes of a scale, enqueued on both orientations' streams behind scale_prepare
void scale_apply(dsa_mat* h, double alpha, const double* d_r, const double* d_c) {
    if (h->col.capacity() <= 0 || h->row.capacity() <= 0) return;
    const int64_t vb = ((d_r ? h->m : 0) + (d_c ? h->n : 0)) * (int64_t)sizeof(double);
    Pma& C = h->col;
    LAUNCH("scale", launch_scale_apply(C.K(), C.V(), C.O(), C.capacity(), C.col_keys, C.h_ctl->table_len, alpha, d_r, h->m, d_c, h->n, true,
                                       stream_nt(C, vb), C.sc.scratch, C.stream));
    Pma& R = h->row;
    LAUNCH("scale", launch_scale_apply(R.K(), R.V(), R.O(), R.capacity(), R.col_keys, R.h_ctl->table_len, alpha, d_c, h->n, d_r, h->m, false,
                                       stream_nt(R, vb), R.sc.scratch, R.stream));
}

}  // namespace host
}  // namespace dsa
