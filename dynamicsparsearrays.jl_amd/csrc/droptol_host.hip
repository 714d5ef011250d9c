// csrc/droptol_host.hip — host side of the in-place pruning of small entries (dsa_mat_droptol[_dev]): argument checks, the scratch
// and pinned words (Pma::drp), the one hand-over per orientation, the control blocks and the root rebalances behind the mark passes.
// Host-only unit: the kernels are in droptol.hip.
// A droptol is two steps so that the entry point (mutate_host.hip) can bump the content epoch between them, as for a scale or a batched
// delete: droptol_prepare (flush, checks, the decide pass: every error, "nothing to drop" and the count-only call with nothing
// modified and every cached plan intact) and droptol_apply (the writes).  Delete-only: no slot is allocated, no table entry changes.
#include "host.h"
#include "droptol.h"

#include <cmath>

namespace dsa {
namespace host {

// Everything of a droptol in front of its first write: the decide pass of both orientations, each on its own stream, and one wait for
// both.  Returns the number of cells the predicate drops; their masks are left in the scratch of each orientation for droptol_apply.
int64_t droptol_prepare(dsa_mat* h, double tol, const double* d_rtol, int64_t nr, const double* d_ctol, int64_t nc) {
    mat_flush(h);
    if (h->fillmode || !h->has_major) fail(DSA_EMODE, "Cannot drop entries in fill mode");
    if (std::isnan(tol)) fail(DSA_EARG, "droptol: tol is NaN");
    if (d_rtol && nr != h->m) fail(DSA_EARG, "nr must equal the number of rows");
    if (d_ctol && nc != h->n) fail(DSA_EARG, "nc must equal the number of columns");
    if (h->col.capacity() <= 0 || h->row.capacity() <= 0) return 0;      // no slot array: nothing is stored
    const int64_t vb = ((d_rtol ? h->m : 0) + (d_ctol ? h->n : 0)) * (int64_t)sizeof(double);
    Pma* const side[2] = {&h->col, &h->row};
    unsigned long long seq[2] = {0, 0};
    for (int o = 0; o < 2; ++o) {
        Pma& P = *side[o];
        ExportArea& A = P.drp;
        A.ensure(P.stream, droptol_scratch_bytes(P.capacity()), 5);      // pinned {error word, count, seq} and the check pass's {error word, seq}
        seq[o] = A.next();
        // colmajor: keys are rows, partitions columns; rowmajor: the other way round
        LAUNCH("droptol (decide)", launch_droptol_decide(P.view(), tol, o == 0 ? d_rtol : d_ctol, o == 0 ? h->m : h->n, o == 0 ? d_ctol : d_rtol,
                                                         o == 0 ? h->n : h->m, stream_nt(P, vb), A.scratch, A.pin, seq[o], P.stream));
    }
    for (int o = 0; o < 2; ++o) wait_handover(*side[o], side[o]->drp.pin + 2, seq[o], "droptol (decide)");
    for (int o = 0; o < 2; ++o) export_verdict(side[o]->drp.pin, "droptol", "a stored entry lies outside size(m)");
    const unsigned long long cc = h->col.drp.pin[1], cr = h->row.drp.pin[1];
    if (cc != cr)
        fail(DSA_EASSERT, "droptol: the two orientations disagree about the entries to drop (" + std::to_string(cc) + " / " + std::to_string(cr) + ")");
    return (int64_t)cc;
}

// The writes, behind droptol_prepare of the same arguments with a count > 0: per orientation, on its own stream, the mark pass and the
// root rebalance of the survivors.  Every semaphore stays: nb_partitions and the tables are as they were.
void droptol_apply(dsa_mat* h, int64_t count) {
    Pma* const side[2] = {&h->col, &h->row};
    for (Pma* P : side) {
        LAUNCH("droptol (mark)", launch_droptol_mark(P->O(), P->capacity(), P->drp.scratch, P->stream));
        P->h_ctl->nb_elements -= count;
        respread(*P);
    }
    for (Pma* P : side) upload_ctl(*P);
}

}  // namespace host
}  // namespace dsa
