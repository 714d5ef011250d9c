// csrc/delbatch_host.hip — host side of the batched delete (dsa_mat_delete_batch[_dev]): argument checks, the scratch and pinned
// words (Pma::del of the own orientation), the two hand-overs, the control blocks and the root rebalances behind the mark passes.
// Host-only unit: the kernels are in delbatch.hip.
// A delete is two steps so that the entry point (mutate_host.hip) can bump the content epoch between them, as for a scale:
// delete_batch_prepare (flush, checks, the validate pass: every error with nothing modified and every cached plan intact) and
// delete_batch_apply (the writes).  The own orientation is the one whose partitions the keys name, the twin the other one.
#include "host.h"
#include "delbatch.h"

#include <climits>

namespace dsa {
namespace host {

// What is left of an orientation after its mark pass, in slot order, spread over [1, capacity] by the root rebalance: the layout
// dsa_mat_rebalance_root gives.  A single leaf is left as it is (root _even_rebalance! is a no-op there, src/pma.jl:96-99), and with
// no cell left there is nothing to move and nothing to clear: the mark pass has cleared every bit (the branch of window_rebalance
// for m = 0 without its launch).  The layout epoch moves in every case: cells are gone.
void respread(Pma& X) {
    Ctl& c = *X.h_ctl;
    if (c.capacity == c.segment_capacity || c.nb_elements <= 0) { ++X.layout_epoch; return; }
    c.stat_rebalances += 1; c.stat_window_slots += c.capacity;
    root_rebalance(X, c.capacity, c.capacity, c.nb_elements, false);
}

// Everything of a batched delete in front of its first write.  Returns the number of matrix entries the delete removes, or -1 for an
// empty list (nothing to do).  Throws DSA_EMODE / DSA_EARG with both orientations untouched.
int64_t delete_batch_prepare(dsa_mat* h, int32_t orientation, const int64_t* d_keys, int64_t n) {
    mat_flush(h);
    if (h->fillmode || !h->has_major) fail(DSA_EMODE, "Cannot delete columns or rows in fill mode");
    if (orientation != DSA_COLMAJOR && orientation != DSA_ROWMAJOR) fail(DSA_EARG, "orientation must be 0 or 1");
    if (n < 0) fail(DSA_EARG, "delete batch: n is negative");
    if (n == 0) return -1;
    if (!d_keys) fail(DSA_EARG, "delete batch: the key list is NULL");
    if (n > INT32_MAX) fail(DSA_EARG, "delete batch: more than 2^31 - 1 keys");
    const bool rows = orientation == DSA_ROWMAJOR;
    Pma& P = rows ? h->row : h->col;
    const char* what = rows ? "row" : "column";
    if (P.capacity() <= 0 || P.h_ctl->table_len <= 0) {   // no slot array or no partition at all: the first key is the offending one
        int64_t k0 = 0;
        HIPCHK(hipMemcpyAsync(&k0, d_keys, sizeof(int64_t), hipMemcpyDeviceToHost, P.stream));
        HIPCHK(hipStreamSynchronize(P.stream));
        fail(DSA_EARG, std::string("delete batch: ") + what + " " + std::to_string(k0) + " is not a live " + what + " of the matrix");
    }
    ExportArea& A = P.del;
    A.ensure(P.stream, delbatch_scratch_bytes(n), 8);     // pinned: {error, first bad key, partitions, cells, seq} and the twin's {error, cells, seq}
    const unsigned long long seq = A.next();
    LAUNCH("delete batch (validate)", launch_delbatch_validate(P.view(), d_keys, n, A.scratch, A.pin, seq, P.stream));
    wait_handover(P, A.pin + 4, seq, "delete batch (validate)");
    const unsigned long long err = __atomic_load_n(A.pin + 0, __ATOMIC_ACQUIRE);
    if (err & 2u) fail(DSA_EASSERT, "delete batch: slot array and partition tables disagree");
    if (err & 1u)
        fail(DSA_EARG, std::string("delete batch: ") + what + " " + std::to_string((long long)A.pin[1]) + " is repeated in the list or is not a live " +
                           what + " of the matrix (absent, already deleted or <= 0)");
    return (int64_t)A.pin[3];
}

// The writes, behind delete_batch_prepare of the same list (its scratch holds the table and the spans): the twin's streaming pass on
// the twin's stream, the own orientation's marks and root rebalance on its own meanwhile; the twin is rebalanced once its count has
// been checked against `cells`.  Returns with both control blocks uploaded and both streams drained.
void delete_batch_apply(dsa_mat* h, int32_t orientation, int64_t n, int64_t cells) {
    const bool rows = orientation == DSA_ROWMAJOR;
    Pma& P = rows ? h->row : h->col;
    Pma& T = rows ? h->col : h->row;
    ExportArea& A = P.del;
    // (the host has waited for the validate pass: the twin's stream needs no event to see the table)
    const unsigned long long seq = A.next();
    const bool twin_cells = cells > 0 && T.capacity() > 0;
    if (twin_cells) {
        // the key stream goes around the cache when it does not fit an XCD's 4 MB L2 beside the table (the rule of scale_host.hip)
        const bool nt = T.capacity() * (int64_t)T.kb() + (int64_t)A.bytes > (3 << 20);
        LAUNCH("delete batch (twin)", launch_delbatch_mark_twin(T.K(), T.O(), T.capacity(), n, nt, (unsigned long long)cells, A.scratch, A.pin + 5,
                                                                seq, T.stream));
    }
    LAUNCH("delete batch (own)", launch_delbatch_mark_own(P.O(), P.sems, P.col_live, n, A.scratch, P.stream));
    P.h_ctl->nb_elements -= cells + n;                    // the cells and the semaphores
    P.h_ctl->nb_partitions -= n;                          // table_len stays: the entries are tombstones (Pma::view: dense = false)
    respread(P);
    if (twin_cells) {
        wait_handover(T, A.pin + 7, seq, "delete batch (twin)");
        if (__atomic_load_n(A.pin + 5, __ATOMIC_ACQUIRE) & 2u) {
            upload_ctl(P);
            fail(DSA_EASSERT, "delete batch: the two orientations disagree about the entries of the listed keys (" + std::to_string(cells) + " / " +
                                  std::to_string((long long)A.pin[6]) + ")");
        }
        T.h_ctl->nb_elements -= cells;                    // every semaphore of the twin stays (src/pcsr.jl:341-351 deletes elements only)
    }
    // (also when the listed partitions were empty: the layout after the call is one rule, whatever the list held)
    if (T.capacity() > 0) respread(T);
    upload_ctl(P);
    upload_ctl(T);
}

}  // namespace host
}  // namespace dsa
