// csrc/assemble_host.hip — host side of the general write from triples in HBM (dsa_mat_assemble[_dev]): argument checks, the key
// scan, the scratch and pinned words (Pma::asmb of the colmajor orientation), the hand-over of the distinct-cell count, the events
// that let the rowmajor stream read what the colmajor stream folded and compacted, and the two halves it drives: update_host.hip on
// the folded cells, insert_host.hip on the cells the update reports missing.  Host-only unit: the kernels are in assemble.hip.
// Two steps, like the halves: assemble_prepare — everything in front of the first write, every error with nothing modified and
// every cached plan intact — and assemble_apply.  Host waits of a call: the key scan, the distinct-cell count, update's verdict, and
// with misses insert's key scan and its two verdicts.  The number of launches does not depend on n.
#include "host.h"
#include "assemble.h"

#include <algorithm>
#include <climits>
#include <cstdio>

namespace dsa {
namespace host {

namespace {

int range_bits(const KeyRange& r) {
    uint64_t x = (uint64_t)r.hi - (uint64_t)r.lo;
    int b = 0;
    while (x) { ++b; x >>= 1; }
    return b;
}

// the rowmajor stream goes on behind what the colmajor stream has enqueued so far
void row_after_col(dsa_mat* h) {
    Pma& C = h->col;
    if (C.ev_asm == nullptr) HIPCHK(hipEventCreateWithFlags(&C.ev_asm, hipEventDisableTiming));
    HIPCHK(hipEventRecord(C.ev_asm, C.stream));
    HIPCHK(hipStreamWaitEvent(h->row.stream, C.ev_asm, 0));
}

// A half failed on entry f.op of the list it was given (I, J, last: that list in the scratch).  The message is rewritten to name the
// cell and the last op of the caller's batch that addresses it: one small read-back, on the error path only.
[[noreturn]] void rethrow_named(dsa_mat* h, const Fail& f, int32_t code, const int64_t* d_I, const int64_t* d_J, const uint32_t* d_last) {
    int64_t cell[2] = {0, 0};
    uint32_t k = 0;
    hipStream_t s = h->col.stream;
    HIPCHK(hipMemcpyAsync(&cell[0], d_I + f.op, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&cell[1], d_J + f.op, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&k, d_last + f.op, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    std::string msg = f.msg;
    const std::string was = op_text((unsigned long long)f.op);
    const std::string now = op_text(k) + ", the last on cell (" + std::to_string(cell[0]) + ", " + std::to_string(cell[1]) + "),";
    const size_t at = msg.find(was);
    if (at != std::string::npos) msg.replace(at, was.size(), now); else msg += " [" + now + "]";
    const size_t colon = msg.find(": ");
    fail(code, "assemble" + (colon != std::string::npos ? msg.substr(colon) : ": " + msg));
}

}  // namespace

// what both forms check before anything is staged or launched (I, J, V: host or device addresses)
void assemble_check_args(dsa_mat* h, int32_t op, const void* I, const void* J, const void* V, int64_t n) {
    if (h->fillmode || !h->has_major) fail(DSA_EMODE, "Cannot assemble triples in fill mode");
    if (op != DSA_UPD_SET && op != DSA_UPD_ADD) fail(DSA_EARG, "assemble: op must be DSA_UPD_SET or DSA_UPD_ADD");
    if (n < 0) fail(DSA_EARG, "assemble: n is negative");
    if (n > 0 && (!I || !J || !V)) fail(DSA_EARG, "assemble: an operand is NULL");
    if (n > INT32_MAX) fail(DSA_EARG, "assemble: more than 2^31 - 1 ops");
}

AssembleCounts assemble_prepare(dsa_mat* h, int32_t op, const int64_t* d_I, const int64_t* d_J, const double* d_V, int64_t n) {
    mat_flush(h);
    assemble_check_args(h, op, d_I, d_J, d_V, n);
    AssembleCounts r;
    if (n == 0) return r;
    const auto t0 = Clock::now();
    Pma& C = h->col;
    // first hand-over: the value ranges of the keys, for the sort and for the reserved keys (every op, also one a later op overrides)
    KeyRange rows, cols;
    bool iz = false, jz = false;
    HIPCHK(device_key_scan(d_I, d_J, n, &rows, &cols, &iz, &jz, C.stream));
    if (!rows.known() || !cols.known()) fail(DSA_EASSERT, "assemble: the key scan returned no range");
    if (rows.lo < 1 || cols.lo < 1) fail(DSA_EKEY, "assemble: a row or column index below 1 (0 is the reserved semaphore key, src/pcsr.jl:23)");
    C.asmb.ensure(C.stream, assemble_scratch_bytes(n), ASM_PIN_WORDS);
    const AsmScratch s = asm_carve(C.asmb.scratch, n);
    const unsigned long long seq = C.asmb.next();
    LAUNCH("assemble (fold)", launch_assemble_fold(d_I, d_J, d_V, n, rows.lo, range_bits(rows), cols.lo, range_bits(cols), op == DSA_UPD_ADD,
                                                   C.asmb.scratch, C.asmb.pin, seq, C.stream));
    // second hand-over: the distinct cells size the halves.  Its word is written by the scan IN FRONT of the fold: the rowmajor
    // stream, on which update_prepare locates, waits for an event behind the fold instead
    row_after_col(h);
    wait_handover(C, C.asmb.pin + ASM_PIN_WORDS - 1, seq, "assemble (fold)");
    const int64_t m = (int64_t)__atomic_load_n(C.asmb.pin, __ATOMIC_ACQUIRE);
    if (m < 1 || m > n) fail(DSA_EASSERT, "assemble: the fold of " + std::to_string(n) + " ops left " + std::to_string(m) + " cells");
    const auto t1 = Clock::now();
    UpdateCounts u{0, 0};
    try {
        u = update_prepare(h, op, DSA_UPD_SKIP_MISSING, s.fI, s.fJ, s.fV, m, s.miss);
    } catch (const Fail& f) {
        if (f.op < 0 || f.op >= m) throw;
        rethrow_named(h, f, f.code, s.fI, s.fJ, s.flast);
    }
    if (u.updated + u.missing != m)
        fail(DSA_EASSERT, "assemble: the update wrote " + std::to_string(u.updated) + " and missed " + std::to_string(u.missing) + " of " +
                              std::to_string(m) + " distinct cells");
    r.distinct = m; r.updated = u.updated; r.missing = u.missing;
    r.rows = rows; r.cols = cols;
    r.folded_V = s.fV; r.missing_V = s.cV;
    const auto t2 = Clock::now();
    if (u.missing > 0) {
        LAUNCH("assemble (compact)", launch_assemble_compact(C.asmb.scratch, n, m, C.stream));
        row_after_col(h);
        try {
            r.ins = insert_prepare(h, s.cI, s.cJ, s.cV, u.missing, 0, nullptr);
        } catch (const Fail& f) {
            if (f.op < 0 || f.op >= u.missing) throw;
            // a cell that update did not find and insert finds stored (or twice) means the halves disagree
            rethrow_named(h, f, f.code == DSA_EARG ? DSA_EASSERT : f.code, s.cI, s.cJ, s.clast);
        }
        if (r.ins.ops != u.missing)
            fail(DSA_EASSERT, "assemble: the update missed " + std::to_string(u.missing) + " cells, the insert creates " + std::to_string(r.ins.ops));
    }
    if (dbg_time())
        fprintf(stderr, "[assemble] n=%lld m=%lld scan + fold %.1f us, update %.1f us, compact + insert %.1f us\n", (long long)n, (long long)m,
                elapsed_us(t0, t1), elapsed_us(t1, t2), elapsed_us(t2));
    return r;
}

// The writes, behind assemble_prepare with something to write.  Per orientation the update's stores and the insert's merge are on
// the same stream: the merge moves the updated values.  With cells created it returns with both streams drained (insert_apply).
void assemble_apply(dsa_mat* h, int32_t op, const AssembleCounts& c) {
    if (c.updated > 0) update_apply(h, op, c.folded_V, c.distinct);
    if (c.missing > 0) insert_apply(h, c.ins, c.missing_V, c.missing);
    // setindex! raises size(m) to the written cell also when it is stored (src/matrix.jl:43-62): a closed fill-mode matrix can hold
    // keys beyond its size
    h->m = std::max(h->m, c.rows.hi);
    h->n = std::max(h->n, c.cols.hi);
}

}  // namespace host
}  // namespace dsa
