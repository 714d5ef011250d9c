// csrc/matwrite_host.hip — what every write to a matrix goes through, in terms of dsa_mat: the builds of both orientations, the batch
// of setindex! calls with its three strategies (both orientations through the batch-parallel rounds; a small batch on two streams; the
// reference's statement order with the host replay of the partition table), the flush of queued single writes, and the delete of one
// column or row.  Host-only unit: everything that works on ONE orientation is in writes_host.hip and build_host.hip; the C entry
// points (argument checks of the ABI + one or two calls into this unit) are in dsa_host.hip.
#include "host.h"

#include <algorithm>
#include <exception>
#include <thread>
#include <vector>

namespace dsa {
namespace host {

namespace {

// The two orientations are independent structures that both only read the caller's arrays: `col` runs on the calling thread, `row`
// beside it on a helper thread when `side_by_side` (the caller's condition: at least two different streams), else behind it on the
// calling thread.  The helper thread binds the handle's device; it is joined before anything is rethrown; an exception of the
// colmajor side wins over one of the rowmajor side.  Returns the time at which the colmajor side was done.
template <class ColFn, class RowFn>
Clock::time_point col_beside_row(dsa_mat* h, bool side_by_side, ColFn&& col, RowFn&& row) {
    if (!side_by_side) { col(); const auto t_col = Clock::now(); row(); return t_col; }
    std::exception_ptr row_exc;
    std::thread row_thread([&] {
        try { bind_device(h->row); row(); }
        catch (...) { row_exc = std::current_exception(); }
    });
    try { col(); }
    catch (...) { row_thread.join(); throw; }
    const auto t_col = Clock::now();
    row_thread.join();
    if (row_exc) std::rethrow_exception(row_exc);
    return t_col;
}

// The sequencer of S is launched on its ops, the ops of R go through the local rounds meanwhile (one wave per op instead of one op
// after the other), then the sequencer is stepped to its end — also when the rounds throw.  Both error codes and progress counts.
struct SeqBesideRounds { int32_t seq_err = 0, rounds_err = 0; int64_t seq_done = 0, rounds_done = 0; };
SeqBesideRounds seq_beside_rounds(Pma& S, const std::vector<Op>& seq_ops, Pma& R, const std::vector<Op>& round_ops) {
    SeqBesideRounds out;
    SeqRun rs;
    seq_start(rs, S, seq_ops);
    try { out.rounds_done = run_ops_parallel(R, round_ops, &out.rounds_err); } catch (...) { while (seq_step(rs)) {} throw; }
    while (seq_step(rs)) {}
    out.seq_err = rs.err; out.seq_done = rs.applied;
    return out;
}

bool parbatch_on() {
    static const bool par = [] { const char* e = dev_env("DSA_PARBATCH"); return !(e && e[0] == '0'); }();
    return par;
}

}  // namespace

// both orientations from (row, col, value) triples that are ALREADY in HBM (they stay the caller's): dynamicsparse(I, J, V) after its
// upload, closefillmode! straight from the device-resident fill buffer.  On failure nothing of the two structures is left behind.
void mat_build_major_dev(dsa_mat* h, const int64_t* dI, const int64_t* dJ, const double* dV, int64_t nnz, bool wide_rows, bool wide_cols,
                         KeyRange rows, KeyRange cols) {
    try {
        const auto ti0 = Clock::now();
        pma_init_common(h->col, true, true);
        pma_init_common(h->row, true, true);
        const auto tb0 = Clock::now();
        if (dbg_time()) fprintf(stderr, "[mat_build_major] handles (streams, control blocks) %.2f ms\n", elapsed_ms(ti0, tb0));
        // large builds: ONE sort of the triples, the rowmajor orientation from the cells colmajor's emit leaves behind (mat_build_both_dev);
        // smaller ones, a shared stream or an injected failure: two independent builds side by side (each waits once for its cell /
        // partition counts)
        if (nnz >= (1 << 16) && h->col.stream != h->row.stream && dev_env("DSA_FAIL_BUILD") == nullptr) {
            const bool both = mat_build_both_dev(h->col, h->row, dJ, dI, dV, nnz, wide_rows, wide_cols, cols, rows);
            if (!both) pma_build_dev(h->row, dI, dJ, dV, nnz, DSA_COMBINE_ADD, 0, 0, wide_cols, rows, cols);
            if (dbg_time()) fprintf(stderr, "[mat_build_major] nnz=%lld both orientations (%s) %.1f ms\n", (long long)nnz, both ? "twin derived" : "general path",
                                    elapsed_ms(tb0));
            h->has_major = true;
            return;
        }
        const auto tb1 = col_beside_row(h, h->col.stream != h->row.stream && nnz > 0,
            [&] { pma_build_dev(h->col, dJ, dI, dV, nnz, DSA_COMBINE_ADD, 0, 0, wide_rows, cols, rows); },       // dynamicsparsecolmajor(I, J, V): partitions = columns, keys = rows
            [&] { pma_build_dev(h->row, dI, dJ, dV, nnz, DSA_COMBINE_ADD, 0, 0, wide_cols, rows, cols); });      // dynamicsparsecolmajor(J, I, V): partitions = rows, keys = columns
        if (dbg_time())
            fprintf(stderr, "[mat_build_major] nnz=%lld colmajor %.1f ms  rowmajor %.1f ms\n", (long long)nnz, elapsed_ms(tb0, tb1), elapsed_ms(tb1));
    } catch (...) {
        // streams, control blocks and whatever slot buffers / tables exist by now (dsa_mat_destroy only looks at them once has_major is set)
        pma_destroy(h->col);
        pma_destroy(h->row);
        throw;
    }
    h->has_major = true;
}

// dynamicsparse(I, J, V): upload + both builds; *rows_out / *cols_out receive the value ranges of the keys
void mat_build_major(dsa_mat* h, const int64_t* I, const int64_t* J, const double* V, int64_t nnz, KeyRange* rows_out, KeyRange* cols_out) {
    int64_t *dI = nullptr, *dJ = nullptr; double* dV = nullptr;
    const auto tup0 = Clock::now();
    HIPCHK(hipSetDevice(g_device));
    try {
        KeyRange rows, cols;
        bool zr = false, zc = false;
        if (nnz > 0) {
            HIPCHK(pool_alloc(reinterpret_cast<void**>(&dI), (size_t)nnz * sizeof(int64_t)));
            HIPCHK(pool_alloc(reinterpret_cast<void**>(&dJ), (size_t)nnz * sizeof(int64_t)));
            HIPCHK(pool_alloc(reinterpret_cast<void**>(&dV), (size_t)nnz * sizeof(double)));
            HIPCHK(hipMemcpy(dI, I, (size_t)nnz * sizeof(int64_t), hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(dJ, J, (size_t)nnz * sizeof(int64_t), hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(dV, V, (size_t)nnz * sizeof(double), hipMemcpyHostToDevice));
            // value ranges (K-build's composite, the storage width of the keys, the size guesses) and the reserved key 0: one pass on
            // the device over the arrays just uploaded — the host never loops over the caller's 10^7 keys
            launch_check(device_key_scan(dI, dJ, nnz, &rows, &cols, &zr, &zc, nullptr), "key scan: ");
        }
        if (dbg_time()) fprintf(stderr, "[mat_build_major] upload of %lld triples from caller memory + key scan %.1f ms\n", (long long)nnz, elapsed_ms(tup0));
        if (rows_out) *rows_out = rows;
        if (cols_out) *cols_out = cols;
        if (zr || zc) check_key(0);
        mat_build_major_dev(h, dI, dJ, dV, nnz, needs_wide(rows), needs_wide(cols), rows, cols);
    } catch (...) { pool_free(dI); pool_free(dJ); pool_free(dV); throw; }      // (a failed build has synchronised and destroyed its streams)
    pool_free(dI); pool_free(dJ); pool_free(dV);
}

// both builds of a fresh handle from triples in HBM with known key ranges (ingest_host.hip), then the SpMV meta prefetch every
// constructor ends with; the caller discards the handle when either throws (mat_discard)
void mat_build_from_dev(dsa_mat* h, const int64_t* dI, const int64_t* dJ, const double* dV, int64_t nnz, KeyRange rows, KeyRange cols) {
    mat_build_major_dev(h, dI, dJ, dV, nnz, needs_wide(rows), needs_wide(cols), rows, cols);
    mat_prefetch_spmv_meta(h);
}

// a handle whose construction failed: whatever exists of the two structures (pma_destroy leaves an empty Pma: calling it again is harmless)
// and the handle itself
void mat_discard(dsa_mat* h) {
    pma_destroy(h->col);
    pma_destroy(h->row);
    delete h;
}

namespace {

// Host replay of ONE partition table (MappedPackedCSC.col_keys + which ids are tombstones) through a batch of writes: which write is
// the first one the reference refuses?  Control logic like the integer density bounds — no slot is read or written here; the device
// executes (and judges) every write.  Follows find(col_keys, col) + addcolumn! + the table half of addpartition!(pcsc, prev)
// (src/pcsr.jl:341-351, 148-169, 114-146): a key that is present changes nothing; a key behind the last entry is pushed; a key whose
// table slot prev+1 is a tombstone reuses it, unless no live id follows (semaphores[0]: BoundsError, :121-125); a key in front of an
// occupied slot shifts the tail of the tables, which asserts on the first tombstone it meets (:129-133).
struct TableReplay {
    std::vector<int64_t> ck; std::vector<uint8_t> live;
    int64_t last_tomb = 0, last_live = 0;          // 1-based index of the last tombstone / the last live entry (0: none)
    void load(Pma& P) {
        const int64_t len = P.h_ctl->table_len;
        ck.resize((size_t)len); live.resize((size_t)len);
        if (len > 0) {
            HIPCHK(hipMemcpyAsync(ck.data(), P.col_keys, (size_t)len * sizeof(int64_t), hipMemcpyDeviceToHost, P.stream));
            HIPCHK(hipMemcpyAsync(live.data(), P.col_live, (size_t)len, hipMemcpyDeviceToHost, P.stream));
            HIPCHK(hipStreamSynchronize(P.stream));
        }
        rescan();
    }
    void rescan() {
        last_tomb = 0; last_live = 0;
        for (int64_t i = (int64_t)live.size(); i >= 1 && (last_tomb == 0 || last_live == 0); --i) {
            if (live[(size_t)i - 1]) { if (last_live == 0) last_live = i; } else if (last_tomb == 0) last_tomb = i;
        }
    }
    // find(col_keys, key) with tombstones (the host twin of d_find_table, csrc/find_dev.h): position of the key or of its predecessor
    int64_t find(int64_t key, bool* exact) const {
        int64_t from = 1, to = (int64_t)ck.size();
        *exact = false;
        while (from <= to) {
            const int64_t mid = (from + to) >> 1;
            int64_t i = mid;
            while (i >= from && !live[(size_t)i - 1]) --i;
            if (i < from) from = mid + 1;
            else {
                const int64_t c = ck[(size_t)i - 1];
                if (c > key) to = i - 1;
                else if (c < key) from = mid + 1;
                else { *exact = true; return i; }
            }
        }
        int64_t i = to;
        while (i > 0 && !live[(size_t)i - 1]) --i;
        return i;
    }
    // a write into partition `key`: 0 when the table accepts it (and the table as it is afterwards), else the reference's error
    int32_t touch(int64_t key) {
        bool exact = false;
        const int64_t prev = find(key, &exact);
        if (exact) return 0;
        const int64_t len = (int64_t)ck.size();
        if (prev == len) { ck.push_back(key); live.push_back(1); last_live = len + 1; return 0; }
        if (!live[(size_t)prev]) {                                  // entry prev + 1 is a tombstone: reuse it
            if (last_live <= prev + 1) return DSA_EBOUNDS;
            ck[(size_t)prev] = key; live[(size_t)prev] = 1;
            if (last_tomb == prev + 1) rescan();
            return 0;
        }
        if (last_tomb >= prev + 1) return DSA_EASSERT;               // the shift of the tail meets a tombstone
        ck.insert(ck.begin() + prev, key); live.insert(live.begin() + prev, (uint8_t)1);
        last_live = len + 1;
        return 0;
    }
};

// setindex! on both orientations for writes [0, n): colmajor[I[k], J[k]] = V[k] / rowmajor[J[k], I[k]] = V[k]  (src/matrix.jl:53-59)
struct SetBatch { const int64_t* I; const int64_t* J; const double* V; int64_t n; };

// size(m) after writes [from, to): a write of a nonzero raises it (src/matrix.jl:44-47)
void grow_size(dsa_mat* h, const SetBatch& b, int64_t from, int64_t to) {
    for (int64_t k = from; k < to; ++k) if (b.V[k] != 0.0) { h->m = std::max(h->m, b.I[k]); h->n = std::max(h->n, b.J[k]); }
}

// the op arrays of the strategies that do not hand the caller's columns to the rounds as they are
void build_ops(const SetBatch& b, std::vector<Op>& oc, std::vector<Op>& orw) {
    oc.resize((size_t)b.n); orw.resize((size_t)b.n);
    for (int64_t k = 0; k < b.n; ++k) {
        oc[(size_t)k] = make_op(OP_MPCSC_SET, b.I[k], b.J[k], b.V[k]);
        orw[(size_t)k] = make_op(OP_MPCSC_SET, b.J[k], b.I[k], b.V[k]);
    }
}

// With tombstones a write can only fail while it CREATES a partition in the middle of the table (addpartition!(pcsc, prev),
// src/pcsr.jl:114-146: the two asserts, and the lookup behind a tombstoned tail).  A batch whose partition keys never decrease and start
// at or behind the last table entry — which must be live — only ever writes to that entry or appends behind it (find() returns the
// last position, addcolumn! takes its push! branch, src/pcsr.jl:148-154): it cannot fail either, and the two orientations may run side
// by side.  That is column generation with deletions: new columns get new, larger ids while old ones are deleted (config 5 + deletecolumn!:
// 445 -> 330 ms).  Anything else with tombstones keeps the reference's statement order (sets_in_reference_order).
bool cannot_fail(Pma& P, const int64_t* part_keys_of_ops, int64_t n) {
    const Ctl& c = *P.h_ctl;
    if (P.view().dense) return true;
    if (c.table_len <= 0 || c.n_pending != 0) return false;
    uint8_t live = 0; int64_t last_key = 0;
    HIPCHK(hipMemcpyAsync(&live, P.col_live + (c.table_len - 1), 1, hipMemcpyDeviceToHost, P.stream));
    HIPCHK(hipMemcpyAsync(&last_key, P.col_keys + (c.table_len - 1), sizeof(int64_t), hipMemcpyDeviceToHost, P.stream));
    HIPCHK(hipStreamSynchronize(P.stream));
    if (!live) return false;
    int64_t running = last_key;
    for (int64_t k = 0; k < n; ++k) { if (part_keys_of_ops[k] < running) return false; running = part_keys_of_ops[k]; }
    return true;
}

// DSA_DBG_TIME: what sets_through_rounds did, the sequencer's stop reasons of the rowmajor side and, in a -DDSA_PROFILE build, its
// shader-clock split
void report_rounds(dsa_mat* h, int64_t n, Clock::time_point t0, Clock::time_point t_col, Clock::time_point t_row, int64_t rounds0) {
    fprintf(stderr, "[mat_apply_sets] n=%lld both orientations %.2f ms (colmajor done after %.2f ms, rowmajor after %.2f ms)  colmajor (par %lld seq %lld ext %lld)  "
            "rowmajor (par %lld seq %lld ext %lld rounds +%lld)\n", (long long)n,
            elapsed_ms(t0), elapsed_ms(t0, t_col), elapsed_ms(t0, t_row), (long long)h->col.stat_par_ops,
            (long long)h->col.stat_seq_ops, (long long)h->col.h_ctl->stat_extends, (long long)h->row.stat_par_ops, (long long)h->row.stat_seq_ops,
            (long long)h->row.h_ctl->stat_extends, (long long)(h->row.stat_par_rounds - rounds0));
    fprintf(stderr, "    rowmajor: sequencer launches %lld  stops by reason [0 unplannable %lld, 1 newcol %lld, 2 limits %lld, 3 shifts %lld, 4 semleaf %lld, "
            "5 window %lld, 6 scan %lld, 7 conflict %lld]\n", (long long)h->row.stat_seq_launches, (long long)h->row.stat_why[0], (long long)h->row.stat_why[1],
            (long long)h->row.stat_why[2], (long long)h->row.stat_why[3], (long long)h->row.stat_why[4], (long long)h->row.stat_why[5],
            (long long)h->row.stat_why[6], (long long)h->row.stat_why[7]);
    if (h->row.h_ctl->prof[7] != 0) {      // -DDSA_PROFILE builds only: shader-clock split of the rowmajor sequencer (cumulative)
        const int64_t* q = h->row.h_ctl->prof;
        const double us = 1.0 / 100.0;                   // s_memtime ticks at 100 MHz
        fprintf(stderr, "    rowmajor sequencer profile (cumulative): kernel %.0f us | %lld matrix writes: table lookup %.0f us, %lld new partitions %.0f us, write in partition %.0f us "
                "[partition end %.0f, find %.0f, insert/shift %.0f, scan+rebalance %.0f (%lld in-block rebalances %.0f us, %lld slots)] | %lld table merges %.0f us\n",
                q[7] * us, (long long)q[4], q[0] * us, (long long)q[5], q[1] * us, q[2] * us, q[11] * us, q[8] * us, q[9] * us, q[10] * us, (long long)q[13], q[12] * us,
                (long long)q[14], (long long)q[6], q[3] * us);
    }
}

// Strategy 1: batch-parallel rounds per orientation (writes to existing columns with disjoint footprints run concurrently; new columns
// and anything else fall back to the sequential sequencer inside run_ops_parallel), which takes the caller's columns as they are.  No
// write can fail, so the host-driven round / sequencer loops of the two orientations run side by side on their own streams.
void sets_through_rounds(dsa_mat* h, const SetBatch& b) {
    const OpBatch bc(OP_MPCSC_SET, b.I, b.J, b.V, b.n), br(OP_MPCSC_SET, b.J, b.I, b.V, b.n);
    int32_t ec = 0, er = 0;
    int64_t dc = 0, dr = 0;
    const int64_t rounds0 = h->row.stat_par_rounds;
    const auto t0 = Clock::now();
    auto t_row = t0;
    const auto t_col = col_beside_row(h, h->col.stream != h->row.stream,
        [&] { dc = run_ops_parallel(h->col, bc, &ec); },
        [&] { dr = run_ops_parallel(h->row, br, &er); t_row = Clock::now(); });
    if (dbg_time()) report_rounds(h, b.n, t0, t_col, t_row, rounds0);
    const int64_t done = std::min(dc, dr);
    grow_size(h, b, 0, std::min(done + 1, b.n));
    if (ec && er && dr < dc) fail(er, err_text(er));      // both halves failed: the rowmajor half of the EARLIER write comes first
    if (ec) fail(ec, err_text(ec));
    if (er) fail(er, err_text(er));
}

// Strategy 2, no tombstones and two streams: a small batch (a column or a few that arrive together, a row).  The orientation in which
// its writes fall into MANY partitions takes the local rounds (one wave per op: k_local_rounds), the one in which they share a few
// partitions — writes into one column are ordered by nature — its sequencer, side by side.  16 writes of a new column: 218 -> ~120 us.
// A batch that is neither shape: the sequencers of both orientations as a pair.
void sets_small_on_two_streams(dsa_mat* h, const SetBatch& b) {
    std::vector<Op> oc, orw;
    build_ops(b, oc, orw);
    if (parbatch_on() && b.n >= 8) {
        std::vector<int64_t> di(b.I, b.I + b.n), dj(b.J, b.J + b.n);
        std::sort(di.begin(), di.end()); std::sort(dj.begin(), dj.end());
        const int64_t ni = std::unique(di.begin(), di.end()) - di.begin(), nj = std::unique(dj.begin(), dj.end()) - dj.begin();
        const bool many_rows = ni >= 2 * nj && ni >= 8, many_cols = !many_rows && nj >= 2 * ni && nj >= 8;
        if (many_rows || many_cols) {
            const SeqBesideRounds r = many_rows ? seq_beside_rounds(h->col, oc, h->row, orw) : seq_beside_rounds(h->row, orw, h->col, oc);
            grow_size(h, b, 0, std::min(std::min(r.rounds_done, r.seq_done) + 1, b.n));
            if (r.seq_err) fail(r.seq_err, err_text(r.seq_err));
            if (r.rounds_err) fail(r.rounds_err, err_text(r.rounds_err));
            return;
        }
    }
    SeqRun rc, rr;
    run_ops_pair(h->col, oc, h->row, orw, rc, rr);
    grow_size(h, b, 0, std::min(std::min(rc.applied, rr.applied) + 1, b.n));
    if (rc.err) fail(rc.err, err_text(rc.err));
    if (rr.err) fail(rr.err, err_text(rr.err));
}

// Strategy 3, tombstones present (or one shared stream): a write that creates a column can fail (src/pcsr.jl:124,132), so the colmajor
// batch runs first and the rowmajor batch is cut at the failing op, like the reference's statement order — still through the
// batch-parallel rounds for everything that is plannable (writes to existing columns); new columns take the sequencer's literal path.
//
// The state after a FAILED batch is the reference's too (round 6; until then colmajor could hold writes behind the failing one):
// the reference stops at write k with colmajor holding writes [0, k] when its rowmajor statement threw, [0, k) when the colmajor one
// did, rowmajor [0, k) either way (src/matrix.jl:43-62).  Colmajor running ahead of rowmajor is only wrong when ROWMAJOR fails, and
// whether a write fails depends on nothing but the partition table (which ids are tombstones: src/pcsr.jl:114-162).  So when the
// rowmajor table holds tombstones the first write it will refuse is found up front by replaying the table — not the slots — on the
// host (TableReplay), and colmajor is not run beyond it.  The device stays the judge: the error code comes from the device, and
// when the device accepts what the replay predicted to fail the loop simply goes on behind it.
void sets_in_reference_order(dsa_mat* h, const SetBatch& b) {
    const int64_t n = b.n;
    std::vector<Op> oc, orw;
    build_ops(b, oc, orw);
    const bool par_seq = parbatch_on() && n >= 128;
    // ops [pos, ...) of one orientation; returns the index in the batch of the first write not applied
    auto apply = [&](Pma& P, const std::vector<Op>& ops, int64_t pos, int32_t* err) {
        return (par_seq ? run_ops_parallel(P, ops, err, true) : run_ops(P, ops, err)) + pos;
    };
    int64_t pos = 0;
    while (pos < n) {
        const int64_t rem = n - pos;
        int64_t f = n;                                                  // first write the rowmajor table refuses (n: none)
        const Ctl& rc = *h->row.h_ctl;
        if (rem > 1 && rc.nb_partitions != rc.table_len) {
            TableReplay tr;
            tr.load(h->row);
            for (int64_t k = pos; k < n; ++k) if (tr.touch(b.I[k]) != 0) { f = k; break; }
        }
        const int64_t end = std::min(n, f + 1);
        std::vector<Op> pc(oc.begin() + pos, oc.begin() + end), pr(orw.begin() + pos, orw.begin() + end);
        int32_t err = 0;
        const int64_t done = apply(h->col, pc, pos, &err);
        // colmajor refused write `done` (<= f): rowmajor gets the writes in front of it — none of which its table refuses
        if (err) pr.resize((size_t)(done - pos));
        int32_t e2 = 0;
        const int64_t d2 = apply(h->row, pr, pos, &e2);
        if (e2 || err) {
            // Which write fails FIRST in the reference's order (colmajor then rowmajor of write 0, of write 1, ...): the rowmajor half of an
            // earlier write d2 < done comes before the colmajor half of write `done`.  (Rounds 1-4 reported the colmajor error regardless:
            // tools/fuzz.py run_tombstones seed 503707, EBOUNDS where the reference throws the AssertionError of src/pcsr.jl:132 three writes earlier.)
            // The failing write had already updated size(m) in the reference (src/matrix.jl:44-47).
            grow_size(h, b, 0, std::min((e2 ? d2 : done) + 1, n));
            fail(e2 ? e2 : err, err_text(e2 ? e2 : err));
        }
        grow_size(h, b, pos, end);
        pos = end;
    }
}

}  // namespace

// setindex! on both orientations for ops [0, n)  src/matrix.jl:53-59.  Without tombstones an OP_MPCSC_SET cannot fail (the reference's
// assert / bounds paths of addpartition! need a deleted partition, App. A.6 (3)), and neither can a batch that only appends behind a
// live last partition (cannot_fail): the two orientations are then updated concurrently.  Otherwise the colmajor batch runs first and
// the rowmajor batch is cut at the failing op, like the reference's statement order.
void mat_apply_sets(dsa_mat* h, const int64_t* I, const int64_t* J, const double* V, int64_t n) {
    const SetBatch b{I, J, V, n};
    const bool no_tombstones = h->col.view().dense && h->row.view().dense;
    const bool side_by_side_ok = no_tombstones || (n >= 128 && cannot_fail(h->col, J, n) && cannot_fail(h->row, I, n));
    if (parbatch_on() && side_by_side_ok && n >= 128) sets_through_rounds(h, b);
    else if (no_tombstones && h->col.stream != h->row.stream) sets_small_on_two_streams(h, b);
    else sets_in_reference_order(h, b);
}

void mat_prefetch_spmv_meta(dsa_mat* h) {
    if (!h->has_major) return;
    prefetch_spmv_meta(h->row);
    prefetch_spmv_meta(h->col);
}

// every C-ABI entry that can change a value or a slot of the matrix: the SpMV plans of both orientations are stale from here on
void mat_content_changed(dsa_mat* h) {
    for (Pma* P : {&h->col, &h->row}) { ++P->content_epoch; spmv_plan_drop(*P); }
}

// Single setindex! calls are write-combined on the host: they are queued (dsa_mat_set) and applied here, in order, at the latest before
// the next call that observes the structure.
void mat_flush(dsa_mat* h) {
    if (h->has_major) bind_device(h->col);
    if (h->pi.empty()) return;
    std::vector<int64_t> i, j; std::vector<double> v;
    i.swap(h->pi); j.swap(h->pj); v.swap(h->pv);       // the queue is empty even if the apply fails
    mat_apply_sets(h, i.data(), j.data(), v.data(), (int64_t)i.size());
    mat_prefetch_spmv_meta(h);
}

// deletecolumn! / deleterow!  src/matrix.jl:95-111: the partition `key` of the own orientation (DSA_COLMAJOR: a column) leaves it, and
// each of its cells leaves the twin.  The element deletes of the twin cannot fail and touch the other structure: with two streams the
// deletepartition! of the own orientation is launched on its sequencer and the twin's deletes — different partitions, mostly disjoint
// footprints — go through the local rounds meanwhile (105 -> 60 us for a column of 16); an empty partition leaves the twin nothing to
// do (the sequencer pair); one shared stream: the twin, then the own orientation.  The twin's error is reported first.
void mat_delete_partition(dsa_mat* h, int32_t orientation, int64_t key) {
    const bool column = orientation == DSA_COLMAJOR;
    Pma& own = column ? h->col : h->row;
    Pma& twin = column ? h->row : h->col;
    const auto t0 = Clock::now();
    std::vector<int64_t> ks; std::vector<double> vals;
    col_view_of(own, key, ks, vals);
    const auto t1 = Clock::now();
    std::vector<Op> ops;
    for (int64_t k : ks) ops.push_back(make_op(OP_MPCSC_SET, key, k, 0.0));     // twin[key, k] = 0
    std::vector<Op> del{make_op(OP_MPCSC_DELETECOLUMN, 0, key, 0.0)};
    struct Report {      // also when the delete throws
        bool on; const char* tag; Clock::time_point a, b; size_t n;
        ~Report() { if (on) fprintf(stderr, "[%s] view %.1f us, %zu twin deletes + deletepartition %.1f us\n", tag, elapsed_us(a, b), n, elapsed_us(b)); }
    } report{dbg_time(), column ? "deletecolumn" : "deleterow", t0, t1, ks.size()};
    int32_t e_twin = 0, e_own = 0;
    if (own.stream != twin.stream && !ops.empty()) {
        const SeqBesideRounds r = seq_beside_rounds(own, del, twin, ops);
        e_twin = r.rounds_err; e_own = r.seq_err;
    } else if (own.stream != twin.stream) {
        SeqRun rt, ro;
        run_ops_pair(twin, ops, own, del, rt, ro);
        e_twin = rt.err; e_own = ro.err;
    } else {
        run_ops(twin, ops, &e_twin);
        if (!e_twin) run_ops(own, del, &e_own);
    }
    if (e_twin) fail(e_twin, err_text(e_twin));
    if (e_own) fail(e_own, err_text(e_own));
}

}  // namespace host
}  // namespace dsa
