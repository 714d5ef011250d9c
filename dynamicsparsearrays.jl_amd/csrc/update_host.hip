// csrc/update_host.hip — host side of the in-place value update (dsa_mat_update_values[_dev]) and of the batched read that stays in
// HBM (dsa_mat_get_batch_dev): argument checks, the scratch and pinned words (Pma::upd), the event that lets the colmajor stream
// resolve behind the rowmajor locate and the one hand-over.  Host-only unit: the kernels are in update.hip.
// An update is two steps so that the entry point (mutate_host.hip) can bump the content epoch between them, as for a scale or a
// droptol: update_prepare (flush, checks, locate + claim + resolve: every error and the call without a winner with nothing modified
// and every cached plan intact) and update_apply (the stores).  Values only: no slot moves, no table entry or counter changes.
#include "host.h"
#include "update.h"

namespace dsa {
namespace host {

namespace {

// `rec` on `from`, and `to` goes on behind it
void stream_after(Pma& rec, hipStream_t from, hipStream_t to) {
    if (rec.ev_upd == nullptr) HIPCHK(hipEventCreateWithFlags(&rec.ev_upd, hipEventDisableTiming));
    HIPCHK(hipEventRecord(rec.ev_upd, from));
    HIPCHK(hipStreamWaitEvent(to, rec.ev_upd, 0));
}

}  // namespace

// what both forms check before anything is staged or launched (I, J, V: host or device addresses)
void update_check_args(dsa_mat* h, int32_t op, int32_t flags, const void* I, const void* J, const void* V, int64_t n) {
    if (h->fillmode || !h->has_major) fail(DSA_EMODE, "Cannot update stored values in fill mode");
    if (op != DSA_UPD_SET && op != DSA_UPD_ADD) fail(DSA_EARG, "update_values: op must be DSA_UPD_SET or DSA_UPD_ADD");
    if ((flags & ~DSA_UPD_SKIP_MISSING) != 0) fail(DSA_EARG, "update_values: unknown flags");
    if (n < 0) fail(DSA_EARG, "update_values: n is negative");
    if (n > 0 && (!I || !J || !V)) fail(DSA_EARG, "update_values: an operand is NULL");
    if (n >= (int64_t(1) << UPD_K_BITS) || h->col.capacity() >= (int64_t(1) << UPD_K_BITS) || h->row.capacity() >= (int64_t(1) << UPD_K_BITS))
        fail(DSA_EARG, "update_values: more than 2^32 - 1 ops or slots");
}

// Everything of an update in front of its first write: both locates, each on its own stream, the claims, the resolve pass and one
// wait.  The slots and winner flags are left in the scratch of the orientations for update_apply.
UpdateCounts update_prepare(dsa_mat* h, int32_t op, int32_t flags, const int64_t* d_I, const int64_t* d_J, const double* d_V, int64_t n,
                            uint8_t* d_missing) {
    mat_flush(h);
    update_check_args(h, op, flags, d_I, d_J, d_V, n);
    if (n == 0) return UpdateCounts{0, 0};
    Pma& C = h->col;
    Pma& R = h->row;
    C.upd.ensure(C.stream, update_scratch_bytes(n, true), UPD_PIN_WORDS);
    R.upd.ensure(R.stream, update_scratch_bytes(n, false), 1);
    const unsigned long long seq = C.upd.next();
    // colmajor: keys are rows, partitions columns; rowmajor: the other way round
    LAUNCH("update (locate)", launch_update_locate(C.view(), d_I, d_J, n, C.upd.scratch, true, C.stream));
    LAUNCH("update (locate)", launch_update_locate(R.view(), d_J, d_I, n, R.upd.scratch, false, R.stream));
    stream_after(R, R.stream, C.stream);
    LAUNCH("update (resolve)", launch_update_resolve(n, C.upd.scratch, R.upd.scratch, (flags & DSA_UPD_SKIP_MISSING) == 0, op == DSA_UPD_ADD,
                                                     d_missing, C.upd.pin, seq, C.stream));
    wait_handover(C, C.upd.pin + UPD_PIN_WORDS - 1, seq, "update (resolve)");
    const unsigned long long* pin = C.upd.pin;
    const unsigned long long err = __atomic_load_n(pin, __ATOMIC_ACQUIRE);
    if (err & UPD_E_ZERO) fail_op(DSA_EKEY, pin[1], "update_values: " + op_text(pin[1]) + " has the key 0, the reserved semaphore key (src/pcsr.jl:23)");
    if (err & UPD_E_BROKEN)
        fail_op(DSA_EASSERT, pin[2], "update_values: the two orientations disagree about " + op_text(pin[2]) + ", or its partition has no semaphore");
    if (err & UPD_E_MISS) fail_op(DSA_EARG, pin[3], "update_values: " + op_text(pin[3]) + " addresses a cell that is not stored");
    if (err & UPD_E_DUP) fail_op(DSA_EARG, pin[4], "update_values: " + op_text(pin[4]) + " adds to a cell that a later op addresses again");
    return UpdateCounts{(int64_t)pin[6], (int64_t)pin[5]};
}

// The stores, behind update_prepare of the same arguments with at least one winner: per orientation, on its own stream.  The
// colmajor stream goes on only behind the rowmajor stores: they read the winner flags in its scratch.
void update_apply(dsa_mat* h, int32_t op, const double* d_V, int64_t n) {
    Pma& C = h->col;
    Pma& R = h->row;
    const UpdScratch sc = upd_carve(C.upd.scratch, n, true), sr = upd_carve(R.upd.scratch, n, false);
    const bool add = op == DSA_UPD_ADD;
    LAUNCH("update (apply)", launch_update_apply(C.K(), C.V(), C.capacity(), d_V, n, sc.slots, sc.win, add, C.stream));
    LAUNCH("update (apply)", launch_update_apply(R.K(), R.V(), R.capacity(), d_V, n, sr.slots, sc.win, add, R.stream));
    stream_after(R, R.stream, C.stream);
}

// A[I[k], J[k]] for n queries in HBM, on the colmajor stream; no host wait
void get_batch_dev(dsa_mat* h, const int64_t* d_I, const int64_t* d_J, int64_t n, double* d_out, uint8_t* d_found) {
    mat_flush(h);
    if (h->fillmode || !h->has_major) fail(DSA_EMODE, "getindex(row, col) is not available in fill mode.");
    if (n < 0) fail(DSA_EARG, "get_batch: n is negative");
    if (n > 0 && (!d_I || !d_J || !d_out)) fail(DSA_EARG, "get_batch: an operand is NULL");
    LAUNCH("get_batch", launch_get_batch_dev(h->col.view(), d_I, d_J, n, d_out, d_found, h->col.stream));
}

}  // namespace host
}  // namespace dsa
