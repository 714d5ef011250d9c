// csrc/insert_host.hip — host side of the batched insert of cells that are not stored yet (dsa_mat_insert_batch[_dev]): argument
// checks, the key scan, the scratch and pinned words (Pma::ins), the hand-over of each orientation, the choice of the capacity, the
// tables and control blocks around the merge.  Host-only unit: the kernels are in insert.hip.
// An insert is two steps so that the entry point (mutate_host.hip) can bump the content epoch between them, as for an update or a
// batched delete: insert_prepare (flush, checks, scan, sort + locate + verdict: every error and the call without a new cell with
// nothing modified and every cached plan intact) and insert_apply (the writes).
#include "host.h"
#include "insert.h"

#include <climits>
#include <cstdio>

namespace dsa {
namespace host {

// what both forms check before anything is staged or launched (I, J, V: host or device addresses)
void insert_check_args(dsa_mat* h, const void* I, const void* J, const void* V, int64_t n, int32_t flags) {
    if (h->fillmode || !h->has_major) fail(DSA_EMODE, "Cannot insert cells in fill mode");
    if ((flags & ~DSA_INS_SKIP_EXISTING) != 0) fail(DSA_EARG, "insert_batch: unknown flags");
    if (n < 0) fail(DSA_EARG, "insert_batch: n is negative");
    if (n > 0 && (!I || !J || !V)) fail(DSA_EARG, "insert_batch: an operand is NULL");
    if (n > INT32_MAX) fail(DSA_EARG, "insert_batch: more than 2^31 - 1 ops");
}

namespace {

// bits that hold every value of [r.lo, r.hi] - r.lo
int range_bits(const KeyRange& r) {
    uint64_t x = (uint64_t)r.hi - (uint64_t)r.lo;
    int b = 0;
    while (x) { ++b; x >>= 1; }
    return b;
}

// the merge of one orientation behind its verdict: `items` new cells and semaphores, `parts` new partitions
void insert_merge(Pma& P, const double* d_V, int64_t n, int64_t items, int64_t parts, bool wide_keys) {
    if (wide_keys) widen_keys(P);
    Ctl& c = *P.h_ctl;
    const int64_t old_cap = c.capacity, m = c.nb_elements + items;
    // _extend!  src/pma.jl:143-151, as often as the root's upper bound asks for
    while (m > c.hi[c.height]) {
        if (c.capacity > INT32_MAX / 2) fail(DSA_EARG, "insert_batch: the array would exceed 2^31 - 1 slots");
        c.capacity *= 2; c.nb_segments *= 2; c.height += 1;
        compute_bounds(P);
        c.stat_extends += 1;
    }
    c.stat_rebalances += 1; c.stat_window_slots += c.capacity;
    ++P.stat_grid_rebalances;
    ensure_capacity_alloc(P, std::max(old_cap, c.capacity));
    ensure_tables(P, c.table_len + parts);
    ++P.layout_epoch;
    const int alt = 1 - P.cur;
    SlotView V = P.view();
    V.capacity = old_cap;
    LAUNCH("insert_batch (merge)", launch_insert_merge(V, d_V, n, P.ins.scratch, P.KA(alt), P.vals[alt], P.occ[alt], c.capacity, m, P.sems, P.col_keys,
                                                       P.col_live, c.table_len + parts, P.stream));
    // bits beyond the new capacity must be zero in the buffer that becomes current (root_rebalance)
    const int64_t first_word = (c.capacity + 63) / 64;
    if (first_word < P.occ_dirty[alt])
        HIPCHK(hipMemsetAsync(P.occ[alt] + first_word, 0, (size_t)(P.occ_dirty[alt] - first_word) * sizeof(uint64_t), P.stream));
    P.occ_dirty[alt] = first_word;
    P.cur = alt;
    c.nb_elements = m;
    c.table_len += parts;
    c.nb_partitions += parts;
}

}  // namespace

InsertCounts insert_prepare(dsa_mat* h, const int64_t* d_I, const int64_t* d_J, const double* d_V, int64_t n, int32_t flags, uint8_t* d_existing) {
    mat_flush(h);
    insert_check_args(h, d_I, d_J, d_V, n, flags);
    InsertCounts r;
    if (n == 0) return r;
    const auto t0 = Clock::now();
    Pma& C = h->col;
    Pma& R = h->row;
    if (C.capacity() < 1 || R.capacity() < 1 || C.capacity() > INT32_MAX || R.capacity() > INT32_MAX)
        fail(DSA_EARG, "insert_batch: an orientation without a slot array, or one of 2^31 slots or more");
    // first hand-over: the value ranges of the keys, for the sort and for the reserved keys
    bool iz = false, jz = false;
    HIPCHK(device_key_scan(d_I, d_J, n, &r.rows, &r.cols, &iz, &jz, C.stream));
    if (!r.rows.known() || !r.cols.known()) fail(DSA_EASSERT, "insert_batch: the key scan returned no range");
    if (r.rows.lo < 1 || r.cols.lo < 1)
        fail(DSA_EKEY, "insert_batch: a row or column index below 1 (0 is the reserved semaphore key, src/pcsr.jl:23)");
    const auto t1 = Clock::now();
    const int ibits = range_bits(r.rows), jbits = range_bits(r.cols);
    C.ins.ensure(C.stream, insert_scratch_bytes(n, C.capacity()), INS_PIN_WORDS);
    R.ins.ensure(R.stream, insert_scratch_bytes(n, R.capacity()), INS_PIN_WORDS);
    const unsigned long long sc = C.ins.next(), sr = R.ins.next();
    // colmajor: partitions are columns, inner keys rows; rowmajor: the other way round.  (The scan has drained the colmajor stream:
    // the rowmajor stream needs no event to see the caller's arrays.)
    LAUNCH("insert_batch (locate)", launch_insert_prepare(C.view(), d_J, d_I, n, r.cols.lo, jbits, r.rows.lo, ibits, C.ins.scratch, d_existing,
                                                          C.ins.pin, sc, C.stream));
    LAUNCH("insert_batch (locate)", launch_insert_prepare(R.view(), d_I, d_J, n, r.rows.lo, ibits, r.cols.lo, jbits, R.ins.scratch, nullptr,
                                                          R.ins.pin, sr, R.stream));
    // second hand-over: the verdicts
    const auto t2 = Clock::now();
    wait_handover(C, C.ins.pin + INS_PIN_WORDS - 1, sc, "insert_batch (locate)");
    wait_handover(R, R.ins.pin + INS_PIN_WORDS - 1, sr, "insert_batch (locate)");
    if (dbg_time())
        fprintf(stderr, "[insert_batch] n=%lld key scan %.1f us, launches %.1f us, wait for the verdicts %.1f us\n", (long long)n, elapsed_us(t0, t1),
                elapsed_us(t1, t2), elapsed_us(t2));
    const unsigned long long* pc = C.ins.pin;
    const unsigned long long* pr = R.ins.pin;
    const unsigned long long ec = __atomic_load_n(pc, __ATOMIC_ACQUIRE), er = __atomic_load_n(pr, __ATOMIC_ACQUIRE);
    const bool strict = (flags & DSA_INS_SKIP_EXISTING) == 0;
    const auto first = [&](unsigned bit, int word) { return (ec & bit) ? pc[word] : pr[word]; };      // the op an error bit names
    if ((ec | er) & INS_E_BROKEN)
        fail_op(DSA_EASSERT, first(INS_E_BROKEN, 4), "insert_batch: the partition of " + op_text(first(INS_E_BROKEN, 4)) + " has no semaphore, or its slots are out of step with the tables");
    if ((ec | er) & INS_E_DUP)
        fail_op(DSA_EARG, first(INS_E_DUP, 1), "insert_batch: " + op_text(first(INS_E_DUP, 1)) + " addresses a cell that an earlier op of the batch creates");
    if (pc[5] != pr[5])
        fail(DSA_EASSERT, "insert_batch: the two orientations disagree about the ops that are already stored (" + std::to_string(pc[5]) + " / " +
                              std::to_string(pr[5]) + ")");
    if (strict && ((ec | er) & INS_E_EXISTS))
        fail_op(DSA_EARG, first(INS_E_EXISTS, 2), "insert_batch: " + op_text(first(INS_E_EXISTS, 2)) + " addresses a cell that is already stored");
    if ((ec | er) & INS_E_MIDDLE) {
        const bool col = (ec & INS_E_MIDDLE) != 0;
        fail_op(DSA_EMODE, col ? pc[3] : pr[3], std::string("insert_batch: ") + op_text(col ? pc[3] : pr[3]) + " creates a " + (col ? "column" : "row") +
                            " that is not behind the last entry of its table (or that entry is deleted): use set_batch");
    }
    if ((int64_t)pc[8] != C.h_ctl->nb_elements || (int64_t)pr[8] != R.h_ctl->nb_elements)
        fail(DSA_EASSERT, "insert_batch: the occupancy bitmap and the element count disagree");
    r.existing = (int64_t)pc[5];
    r.ops = n - r.existing;
    r.items[0] = (int64_t)pc[6]; r.parts[0] = (int64_t)pc[7];
    r.items[1] = (int64_t)pr[6]; r.parts[1] = (int64_t)pr[7];
    if (r.items[0] - r.parts[0] != r.ops || r.items[1] - r.parts[1] != r.ops)
        fail(DSA_EASSERT, "insert_batch: the orientations disagree about the number of new cells");
    return r;
}

// The writes, behind insert_prepare of the same arguments with at least one new cell: per orientation, on its own stream.  Returns
// with both control blocks uploaded and both streams drained.
void insert_apply(dsa_mat* h, const InsertCounts& c, const double* d_V, int64_t n) {
    // colmajor keeps rows as keys, rowmajor columns; a partition key lives in the tables (64 bits always)
    const auto t0 = Clock::now();
    insert_merge(h->col, d_V, n, c.items[0], c.parts[0], !h->col.wide && !key_fits32(c.rows.hi));
    insert_merge(h->row, d_V, n, c.items[1], c.parts[1], !h->row.wide && !key_fits32(c.cols.hi));
    h->m = std::max(h->m, c.rows.hi);
    h->n = std::max(h->n, c.cols.hi);
    const auto t1 = Clock::now();
    upload_ctl(h->col);
    upload_ctl(h->row);
    if (dbg_time())
        fprintf(stderr, "[insert_batch] merge launches %.1f us, control blocks up and both streams drained %.1f us\n", elapsed_us(t0, t1), elapsed_us(t1));
}

}  // namespace host
}  // namespace dsa
