// csrc/writes_host.hip — the write path of one Pma, host side: a batch of ops and its upload, the yield loop around the on-device
// sequencer (a resumable state machine, so that two structures can run theirs side by side) and the driver of the batch-parallel rounds.
// Host-only unit: launches go through the launch_* functions of the kernel units.
#include "host.h"

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>

namespace dsa {
namespace host {

static std::atomic<bool> g_models_off{false};      // an append-replay model kernel could not be launched on this device (LDS): per-op replay only from then on

static void ensure_ops(Pma& P, int64_t n) {
    P.breaks_valid = false;
    if (n <= P.ops_cap) return;
    HIPCHK(hipStreamSynchronize(P.stream));                  // (a pooled block is handed out again at once: nothing may still read the old one)
    pool_free(P.d_ops); pool_free(P.d_breaks);
    P.d_ops = nullptr; P.d_breaks = nullptr;
    P.ops_cap = std::max<int64_t>(n, 1024);
    HIPCHK(pool_alloc(reinterpret_cast<void**>(&P.d_ops), (size_t)P.ops_cap * sizeof(Op)));
    HIPCHK(pool_alloc(reinterpret_cast<void**>(&P.d_breaks), (size_t)(P.ops_cap / 64 + 8) * sizeof(uint64_t)));
}
// the ops of a batch into d_ops (stream-ordered; the host arrays must stay alive until the batch has finished — every batch waits)
static void upload_batch(Pma& P, const OpBatch& B) {
    const int64_t n = B.n;
    if (B.ops != nullptr) {
        HIPCHK(hipMemcpyAsync(P.d_ops, B.ops, (size_t)n * sizeof(Op), hipMemcpyHostToDevice, P.stream));
        return;
    }
    if (n > P.opsrc_cap) {
        HIPCHK(hipStreamSynchronize(P.stream));
        pool_free(P.d_opsrc); P.d_opsrc = nullptr;
        P.opsrc_cap = std::max<int64_t>(n, P.ops_cap);
        HIPCHK(pool_alloc(reinterpret_cast<void**>(&P.d_opsrc), (size_t)P.opsrc_cap * 3 * sizeof(int64_t)));
    }
    int64_t* da = P.d_opsrc; int64_t* db = P.d_opsrc + P.opsrc_cap; double* dv = reinterpret_cast<double*>(P.d_opsrc + 2 * P.opsrc_cap);
    HIPCHK(hipMemcpyAsync(da, B.a, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, P.stream));
    if (B.b) HIPCHK(hipMemcpyAsync(db, B.b, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, P.stream));
    HIPCHK(hipMemcpyAsync(dv, B.v, (size_t)n * sizeof(double), hipMemcpyHostToDevice, P.stream));
    LAUNCH("make ops", launch_make_ops(da, B.b ? db : nullptr, dv, B.kind, n, P.d_ops, P.stream));
}

// the n ops just uploaded into d_ops: where an append run cannot continue (read by the sequencer's run detection), enqueued behind the
// upload.  Vectors and MappedPackedCSC only — a plain PackedCSC has no runs
static void enqueue_op_breaks(Pma& P, int64_t n) {
    P.breaks_valid = false;
    if (P.occ_old == nullptr || n < 64 || (P.has_sems && !P.has_cols)) return;
    LAUNCH("op breaks", launch_op_breaks(P.d_ops, n, P.has_cols ? 1 : 0, P.d_breaks, P.stream));
    P.breaks_valid = true;
}

static int32_t seq_err_to_status(int32_t e) { return e == 0 ? DSA_EASSERT : e; }

const char* err_text(int32_t e) {
    switch (e) {
        case DSA_EARG: return "column does not exist.";
        case DSA_EBOUNDS: return "cannot access partition at this index";
        case DSA_EDELETED: return "The partition has been deleted.";
        case DSA_EFULL: return "No empty cell to insert a new element.";
        case DSA_EASSERT: return "reference assertion failed (tombstoned partition in the way)";
        default: return "sequencer error";
    }
}

static void ensure_key_width(Pma& P, const OpBatch& B) {
    if (P.wide) return;
    if (B.ops != nullptr) {
        for (int64_t k = 0; k < B.n; ++k) {
            const Op& o = B.ops[k];
            if ((o.kind == OP_VEC_SET || o.kind == OP_PCSC_SET || o.kind == OP_MPCSC_SET) && !key_fits32(o.a)) { widen_keys(P); return; }
        }
        return;
    }
    for (int64_t k = 0; k < B.n; ++k) if (!key_fits32(B.a[k])) { widen_keys(P); return; }
}

// ---- the yield loop around the device sequencer, as a resumable state machine so that the two orientations of a
// matrix can run their sequencers concurrently on their own streams ------------------------------------------------
// Pending partition-table entries (created by the running batch at the end of the tables, Ctl::n_pending) back into key order:
// the grid-wide pass of tables.hip, stream-ordered, no host wait.  h_ctl->table_cap must be current.
static void merge_tables(Pma& P) {
    if (!P.has_cols) return;
    const int64_t cap = P.h_ctl->table_cap;
    if (P.tmerge_cap < cap) {
        if (P.tmerge.sems2) HIPCHK(hipFree(P.tmerge.sems2));          // hipFree waits for the work that may still use them
        if (P.tmerge.keys2) HIPCHK(hipFree(P.tmerge.keys2));
        P.tmerge.sems2 = P.tmerge.keys2 = nullptr; P.tmerge_cap = 0;
        HIPCHK(hipMalloc(&P.tmerge.sems2, (size_t)cap * sizeof(int64_t)));
        HIPCHK(hipMalloc(&P.tmerge.keys2, (size_t)cap * sizeof(int64_t)));
        P.tmerge_cap = cap;
    }
    if (!P.tmerge.pkey) {
        HIPCHK(hipMalloc(&P.tmerge.pkey, (size_t)(3 * 1024 + 8) * sizeof(int64_t)));
        P.tmerge.pdst = P.tmerge.pkey + 1024; P.tmerge.psem = P.tmerge.pkey + 2048; P.tmerge.hdr = P.tmerge.pkey + 3072;
    }
    ++P.layout_epoch;
    if (P.h_ctl->n_pending > TABLE_PEND_MAX) fail(DSA_EASSERT, "more pending partition-table entries than the merge takes (internal invariant)");
    LAUNCH("table merge", launch_table_merge(P.sems, P.col_keys, P.col_live, P.V(), P.d_ctl, P.tmerge, cap, P.stream));
    P.h_ctl->n_pending = 0;
    P.stat_table_merges += 1;
}

// Hand-over of a launch's result through pinned memory (parbatch.hip: k_publish; the sequencer does it in its own epilogue): the last kernel of the launch
// writes the control block (and the round state) into the host's pinned mirrors and then a number into P.h_pub; the host polls for
// that number instead of issuing device-to-host copies and synchronising the stream (dsa_dev.h: wait_pinned_seq).
static unsigned int next_publish_seq(Pma& P) {
    if (++P.pub_seq == 0) P.pub_seq = 1;
    return P.pub_seq;
}
// the burst number k_publish / the sequencer's epilogue write is the low 32 bits of P.h_pub
static void wait_published(Pma& P) { wait_handover(P, P.h_pub, P.pub_seq, "device work", 0xffffffffull); }

static thread_local double g_seq_launch_ms = 0;
static void seq_launch(SeqRun& r, bool upload = true) {
    Pma& P = *r.P;
    struct T { Clock::time_point t0 = Clock::now(); ~T() { g_seq_launch_ms += elapsed_ms(t0); } } timer;
    // pinned h_ctl: H2D, kernel and D2H are stream-ordered; the host does not touch h_ctl until the next synchronize
    if (upload) HIPCHK(hipMemcpyAsync(P.d_ctl, P.h_ctl, sizeof(Ctl), hipMemcpyHostToDevice, P.stream));
    ++P.layout_epoch;
    const unsigned int seq = next_publish_seq(P);       // the sequencer hands its control block back itself
    LAUNCH("sequencer", launch_sequencer(P.K(), P.V(), P.O(), P.has_sems ? P.sems : nullptr, P.has_cols ? P.col_keys : nullptr,
                                         P.has_cols ? P.col_live : nullptr, P.d_ctl, P.d_ops, r.n, std::max(r.n, r.n_avail),
                                         P.occ_old != nullptr, P.breaks_valid ? P.d_breaks : nullptr, P.h_ctl, P.h_pub, seq, P.stream));
}

void seq_start(SeqRun& r, Pma& P, const std::vector<Op>& ops) {
    r = SeqRun();
    r.P = &P; r.ops = &ops; r.n = (int64_t)ops.size();
    if (r.n == 0) return;
    ensure_key_width(P, ops);
    ensure_ops(P, r.n);
    HIPCHK(hipMemcpyAsync(P.d_ops, ops.data(), (size_t)r.n * sizeof(Op), hipMemcpyHostToDevice, P.stream));
    enqueue_op_breaks(P, r.n);
    P.h_ctl->next_op = 0; P.h_ctl->status = 0; P.h_ctl->err = 0; P.h_ctl->no_run_at = -1;
    r.active = true;
    seq_launch(r);
}

// waits for the running kernel of `r`, services its yield and relaunches; returns false once the batch is finished
// dev (DSA_DBG_SPLIT): where a sequencer chunk spends its wall clock — waiting for the device / host work per kind of yield
namespace {
static thread_local double g_seq_wait_ms = 0, g_seq_host_ms[8] = {0};
struct SeqStepTimer {
    Clock::time_point t0; int kind;
    SeqStepTimer(int k) : t0(Clock::now()), kind(k) {}
    ~SeqStepTimer() { g_seq_host_ms[kind & 7] += elapsed_ms(t0); }
};
}  // namespace
bool seq_step(SeqRun& r) {
    if (!r.active) return false;
    Pma& P = *r.P;
    {
        const auto tw0 = Clock::now();
        wait_published(P);
        g_seq_wait_ms += elapsed_ms(tw0);
    }
    Ctl& c = *P.h_ctl;
    SeqStepTimer timer(c.status);
    switch (c.status) {
        case SEQ_DONE:
            r.applied = std::max(r.n, c.next_op); r.active = false;
            if (!r.defer_merge && c.n_pending > 0) merge_tables(P);
            return false;
        case SEQ_ERROR:
            r.err = seq_err_to_status(c.err); r.applied = c.next_op; r.active = false;
            if (!r.defer_merge && c.n_pending > 0) merge_tables(P);
            return false;
        case SEQ_Y_REBALANCE:
            window_rebalance(P, c.y_ws, c.y_we, c.y_m);
            break;
        case SEQ_Y_EXTEND: {       // _extend!  src/pma.jl:143-151 then _even_rebalance!(1, capacity, count)
            const int64_t old_cap = c.capacity;
            c.capacity *= 2; c.nb_segments *= 2; c.height += 1;
            compute_bounds(P);
            c.stat_extends += 1; c.stat_rebalances += 1; c.stat_window_slots += c.capacity;
            root_rebalance(P, old_cap, c.capacity, c.y_m, false);
            break;
        }
        case SEQ_Y_SHRINK: {       // pack! + _shrink!  src/pma.jl:135-139,153-161 then _even_rebalance!
            const int64_t old_cap = c.capacity;
            c.capacity /= 2; c.nb_segments /= 2; c.height -= 1;
            compute_bounds(P);
            c.stat_shrinks += 1; c.stat_rebalances += 1; c.stat_window_slots += c.capacity;
            root_rebalance(P, old_cap, c.capacity, c.y_m, false);
            break;
        }
        case SEQ_Y_TABLE_GROW:
            ensure_tables(P, c.table_len + 1);
            break;
        case SEQ_Y_APPEND_RUN: {
            if (dev_env("DSA_DBG_RUN") && c.dbg[4])
                fprintf(stderr, "[previous append run] ops=%lld slow=%lld fast=%.1fus slow=%.1fus shader clock %.0f MHz | model v2: entries %lld ops %lld wide events %lld "
                        "pattern misses %lld exits [end %lld, word full %lld, word empty %lld, wider level %lld]\n", (long long)c.dbg[4],
                        (long long)c.dbg[0], c.dbg[2] / 100.0, c.dbg[3] / 100.0, c.dbg[5] ? 100.0 * c.dbg[1] / c.dbg[5] : 0.0,
                        (long long)c.prof[8], (long long)c.prof[9], (long long)c.prof[10], (long long)c.prof[11], (long long)c.prof[12], (long long)c.prof[13],
                        (long long)c.prof[14], (long long)c.prof[15]);
            if (dev_env("DSA_DBG_RUN") && c.dbg[4])
                fprintf(stderr, "    model v2: %lld in-word ops simulated one by one; %lld epoch jumps; %lld wide events computed (not memoised) in %.1f us; whole model %.1f us (shader clock)\n", (long long)c.prof[3], (long long)c.prof[4],
                        (long long)c.prof[5], c.prof[6] / 2400.0, c.prof[7] / 2400.0);
            // save the bitmap, replay the run on the live bitmap, move the cells; all stream-ordered, no host wait.  The
            // device control block is authoritative afterwards (next_op, nb_elements, tables, statistics): no upload on relaunch.
            const int64_t words = (c.capacity + 63) / 64;
            const int64_t i0 = c.y_ws, R = c.y_m, n0 = c.y_we;
            hipError_t e;
            if (P.has_cols) {
                // MappedPackedCSC run: at most R new columns; expand the ops into the cell stream (semaphore cells included)
                ensure_tables(P, c.table_len + R + 1);
                if (2 * R + 1024 > P.run_cap) {
                    if (P.run_cells) hipFree(P.run_cells);
                    if (P.run_flags) hipFree(P.run_flags);
                    P.run_cap = std::max<int64_t>(2 * R + 1024, 1 << 16);
                    HIPCHK(hipMalloc(&P.run_cells, (size_t)P.run_cap * sizeof(Op)));
                    HIPCHK(hipMalloc(&P.run_flags, (size_t)(P.run_cap / 64 + 32) * sizeof(uint64_t)));
                }
                if (!P.run_out) HIPCHK(hipMalloc(&P.run_out, 2 * sizeof(int64_t)));
                HIPCHK(hipMemcpyAsync(P.d_ctl, P.h_ctl, sizeof(Ctl), hipMemcpyHostToDevice, P.stream));     // table_cap may have grown
                LAUNCH("run expand", launch_run_expand(P.d_ops, i0, R, P.d_ctl, P.col_keys, P.col_live, P.run_cells, P.run_flags, P.run_out, P.stream));
            }
            HIPCHK(hipMemcpyAsync(P.occ_old, P.O(), (size_t)words * sizeof(uint64_t), hipMemcpyDeviceToDevice, P.stream));
            if (!P.run_memo) {                  // the memo of k_append_run (appendrun.hip), then the 8 result words of k_append_model3
                HIPCHK(hipMalloc(&P.run_memo, append_run_memo_bytes() + 8 * sizeof(int64_t)));
                HIPCHK(hipMemsetAsync(P.run_memo, 0, append_run_memo_bytes() + 8 * sizeof(int64_t), P.stream));
            }
            // the count-only replay first (appendmodel.hip); what it cannot take — short runs, small segments, a tail outside the last
            // leaf — and whatever it leaves is replayed per op by k_append_run.  DSA_MODEL3=0: per-op replay only (A/B, coverage)
            static const bool model3 = [] { const char* v = dev_env("DSA_MODEL3"); return !(v && v[0] == '0'); }();
            // (typed runs on segments below 16 slots are not count-only — appendmodel.hip — and runs below its minimum length do not pay:
            //  no launch for them)
            const bool m3_takes = model3 && !g_models_off.load() && R >= 512 && (P.has_cols ? c.segment_capacity >= 16 : c.segment_capacity >= 2) && c.capacity >= 65536;
            // typed runs on 8-slot segments (a matrix grown from the empty one: BASELINE config 5) are not count-only; their replay is the
            // per-epoch model of appendmodel.hip (k_append_model5).  DSA_MODEL5=0: per-op replay only (A/B, coverage)
            static const bool model5 = [] { const char* v = dev_env("DSA_MODEL5"); return !(v && v[0] == '0'); }();
            const bool m5_takes = model5 && !g_models_off.load() && !m3_takes && P.has_cols && c.segment_capacity == 8 && R >= 64 && c.capacity >= 256;
            int64_t* m3_out = (m3_takes || m5_takes) ? reinterpret_cast<int64_t*>(reinterpret_cast<char*>(P.run_memo) + append_run_memo_bytes()) : nullptr;
            if (m3_takes) {
                e = launch_append_model3(P.O(), P.d_ctl, R, P.has_cols ? P.run_flags : nullptr, P.has_cols ? P.run_out : nullptr, m3_out, P.stream);
            } else if (m5_takes) {
                e = launch_append_model5(P.O(), P.d_ctl, R, P.run_flags, P.run_out, m3_out, P.stream);
            }
            if ((m3_takes || m5_takes) && e != hipSuccess) {
                // The models need 140 KB of LDS per workgroup (gfx950 has 160): on a part that refuses the launch (hipFuncSetAttribute /
                // launch error) the run is not lost — the per-op replay takes all of it, and the models stay off for the process.  Only the
                // codes such a refusal produces are taken that way (and said once on stderr: config 5 is several times slower without the
                // models); anything else — a sticky error of earlier work on the stream, out of memory — is a failure like everywhere else.
                (void)hipGetLastError();
                if (e != hipErrorInvalidValue && e != hipErrorLaunchOutOfResources && e != hipErrorInvalidConfiguration && e != hipErrorSharedObjectInitFailed)
                    fail(DSA_EHIP, std::string("append model launch: ") + hipGetErrorString(e));
                if (!g_models_off.exchange(true))
                    fprintf(stderr, "libdsa_hip: append-replay models disabled for this process (%s): per-op replay from now on\n", hipGetErrorString(e));
                m3_out = nullptr;
            }
            LAUNCH("append run", launch_append_run(P.O(), P.d_ctl, i0, R, P.has_cols ? P.run_flags : nullptr, P.has_cols ? P.run_out : nullptr, P.run_memo, m3_out, P.stream));
            permute_run(P, P.has_cols ? P.run_cells : P.d_ops, P.has_cols ? 0 : i0, n0);
            if (m3_out != nullptr && dev_env("DSA_DBG_RUN")) {
                int64_t o[8];
                HIPCHK(hipMemcpyAsync(o, m3_out, sizeof(o), hipMemcpyDeviceToHost, P.stream));
                HIPCHK(hipStreamSynchronize(P.stream));
                fprintf(stderr, "[append model %s] run of %lld ops: placed %lld status %lld reason %lld | events above the tables %lld, table levels %lld | counts %.1f us tables %.1f us driver %.1f us\n",
                        m5_takes ? "v5 (typed epochs)" : "v3", (long long)R, (long long)o[0], (long long)o[1], (long long)o[2], (long long)o[3], (long long)o[4], o[5] / 100.0, o[6] / 100.0, o[7] / 100.0);
            }
            if (++r.guard > 4 * r.n + 1000000) fail(DSA_EASSERT, "sequencer made no progress");
            seq_launch(r, false);
            return true;
        }
        default:
            fail(DSA_EASSERT, "unknown sequencer status");
    }
    if (++r.guard > 4 * r.n + 1000000) fail(DSA_EASSERT, "sequencer made no progress");
    seq_launch(r);
    return true;
}

// Runs `ops` in order on the device.  Returns the number of ops fully applied; *err receives the
// status of the failing op (0 if all were applied).
int64_t run_ops(Pma& P, const std::vector<Op>& ops, int32_t* err) {
    SeqRun r;
    seq_start(r, P, ops);
    while (seq_step(r)) {}
    *err = r.err;
    return r.applied;
}

// Batch-parallel execution of vector writes (parbatch.hip): rounds of plan / resolve / apply for the prefix of ops whose
// footprints are pairwise disjoint; the op that cuts a short prefix (and a growing chunk after it while prefixes stay
// short: ascending appends, hammering one key) goes through the sequential sequencer.  Same final state as run_ops.
int64_t run_ops_parallel(Pma& P, const OpBatch& ops, int32_t* err, bool can_fail) {
    *err = 0;
    const int64_t n = ops.n;
    if (n == 0) return 0;
    constexpr int GMAX = ROUND_GMAX, MIN_PREFIX = 4, ROUNDS_PER_SYNC = 12, ROUNDS_SHORT = 3;
    constexpr int64_t MERGE_AT = 256;       // pending table entries (of at most 1024) that trigger the grid-wide merge between launches
    ensure_key_width(P, ops);
    ensure_ops(P, n);
    {
        const auto tu0 = Clock::now();
        upload_batch(P, ops);
        enqueue_op_breaks(P, n);
        static const bool dbg_up = dev_env("DSA_DBG_SPLIT") != nullptr;
        if (dbg_up) fprintf(stderr, "  [run_ops_parallel] upload of %lld ops (%.1f MB, pageable): %.3f ms on the host\n", (long long)n, n * sizeof(Op) / 1e6, elapsed_ms(tu0));
    }
    if (!P.d_plans) {
#ifdef DSA_FP_CHECK
        HIPCHK(hipMalloc(&P.d_plans, (size_t)GMAX * (sizeof(Plan) + FP_BYTES_PER_OP)));      // + the recorded sets of the footprint check (parbatch.hip)
        HIPCHK(hipMemsetAsync(P.d_plans, 0, (size_t)GMAX * (sizeof(Plan) + FP_BYTES_PER_OP), P.stream));
#else
        HIPCHK(hipMalloc(&P.d_plans, (size_t)GMAX * sizeof(Plan)));
#endif
        HIPCHK(hipMalloc(&P.d_pend, (size_t)2 * GMAX * sizeof(PendOp)));
        HIPCHK(hipMemsetAsync(P.d_pend, 0, (size_t)2 * GMAX * sizeof(PendOp), P.stream));
        HIPCHK(hipMalloc(&P.d_bufs, sizeof(DevBufs)));
        HIPCHK(hipHostMalloc(&P.h_bufs, sizeof(DevBufs), hipHostMallocDefault));
        std::memset(P.h_bufs, 0, sizeof(DevBufs));
        HIPCHK(hipMalloc(&P.d_rs, sizeof(RoundState)));
        HIPCHK(hipHostMalloc(&P.h_rs, sizeof(RoundState), hipHostMallocDefault));
    }
    P.h_ctl->next_op = 0; P.h_ctl->status = 0; P.h_ctl->err = 0; P.h_ctl->no_run_at = -1;
    upload_ctl(P);
    constexpr int64_t SEQ_CHUNK0 = 8, BARRIER_CHUNK0 = 1;
    int64_t i = 0, seq_chunk = SEQ_CHUNK0;
    // run-ahead (parbatch.hip): a round applies every op that conflicts with no earlier one, the deferred ones wait in a pending list in
    // front of the fresh ops.  Only where no op can fail (a failing op must find exactly the ops in front of it applied): no tombstones,
    // not the cut batches of the tombstone path.  DSA_RUN_AHEAD=0: the prefix rule of rounds 2-5 (A/B).
    static const bool run_ahead_on = [] { const char* e = dev_env("DSA_RUN_AHEAD"); return !(e && e[0] == '0'); }();
    const bool run_ahead = run_ahead_on && !can_fail && P.view().dense;
    int np = 0, cur = 0;                    // pending ops of the rounds and which half of d_pend holds them
    bool drain = false;                     // the next bursts work on the pending list alone ...
    int after_drain = 0;                    // ... and then: 1 switch to the local rounds, 2 the sequencer takes the chunk at the cursor
    int G = 256;
    int ema = 16 * 16;                      // RoundState::ema, carried across the bursts of the batch
    // local rounds (parbatch.hip: k_local_rounds) while the prefixes are short; a small array starts with them
    static const bool local_ok = [] { const char* e = dev_env("DSA_LOCAL_ROUNDS"); return !(e && e[0] == '0'); }();
    constexpr int LOCAL_ROUNDS = 2048, LOCAL_BELOW = 6;
    bool use_local = local_ok && (P.h_ctl->capacity <= (1 << 16) || n <= 64);      // (a handful of ops: one launch of the persistent workgroup, not a burst graph)
    // a burst that stops in its first rounds (short conflict-free prefix, barrier op) leaves the rest of its graph as no-op
    // launches (~2.5 us each, four per round): after such a stop the next burst is a short one, until one runs to its end
    int burst_rounds = ROUNDS_PER_SYNC;
    static const bool dbg_split = dev_env("DSA_DBG_SPLIT") != nullptr;
    double t_burst = 0, t_seq = 0, t_local = 0; int64_t n_burst = 0, n_seq = 0, n_yield = 0, n_local = 0, r_local = 0, o_local = 0;
    int64_t dbg_detour[32] = {0};
    // A batch that starts like an append run — ascending keys (vector) / ascending (column, row) pairs (MappedPackedCSC) — goes to the
    // sequencer first, which detects the run (or, when the keys are not above the last cell after all, applies a few ops and hands
    // back to the rounds): a burst of rounds on ascending appends plans and applies one op per round (0.37 ms for nothing at 100 k ops)
    bool seq_first = false;
    if (P.occ_old != nullptr && n >= 64 && (!P.has_sems || P.has_cols)) {
        const int64_t probe = std::min<int64_t>(n, 256);
        seq_first = true;
        for (int64_t j = 0; j < probe && seq_first; ++j) {
            const Op o = ops.at(j);
            if (o.v == 0.0 || o.kind != (P.has_cols ? OP_MPCSC_SET : OP_VEC_SET)) seq_first = false;
            else if (j > 0) {
                const Op q = ops.at(j - 1);
                seq_first = P.has_cols ? (o.b > q.b || (o.b == q.b && o.a > q.a)) : o.a > q.a;
            }
        }
    }
    while (i < n || np > 0) {
        const auto tb0 = Clock::now();
        bool to_sequencer = seq_first;
        if (!seq_first) {
        // ---- a burst of rounds driven by the device-resident cursor; one host synchronisation per burst
        RoundState& rs = *P.h_rs;
        std::memset(&rs, 0, sizeof(rs));
        static const int tight = [] { const char* e = dev_env("DSA_TIGHT"); return e ? atoi(e) : 3; }();
        rs.cursor = i; rs.limit = n; rs.G = G; rs.min_prefix = MIN_PREFIX; rs.ema = ema; rs.tight = tight;
        rs.cursor_n = i; rs.np = rs.np_n = np; rs.cur = rs.cur_n = cur; rs.run_ahead = run_ahead ? 1 : 0; rs.drain = drain ? 1 : 0; rs.pend0 = i;
#ifdef DSA_FP_CHECK
        {   // the footprint-check build: DSA_FP_MODE = 1 recorded read / touch sets (default), 2 sequential shadow re-plan, 0 neither
            static const int fp_mode = [] { const char* e = dev_env("DSA_FP_MODE"); return e ? atoi(e) : 1; }();
            rs.tight |= fp_mode == 2 ? FP_MODE_SHADOW : (fp_mode == 1 ? FP_MODE_SETS : 0);
        }
#endif
        // the burst hands its result back through pinned memory (k_publish) and the host polls for the burst number
        rs.seq = (int32_t)next_publish_seq(P);
        const BurstPublish pub{P.h_rs, P.h_ctl, P.h_pub};
        HIPCHK(hipMemcpyAsync(P.d_rs, P.h_rs, sizeof(RoundState), hipMemcpyHostToDevice, P.stream));
        {
            ++P.layout_epoch;
            // (every burst is followed by a stream wait, so the pinned mirror is never rewritten under a copy in flight)
            const DevBufs bufs_now{P.K().p, P.V(), P.O(), P.has_sems ? P.sems : nullptr, P.has_cols ? P.col_keys : nullptr,
                                   P.has_cols ? P.col_live : nullptr, P.wide ? 1 : 0, 0, P.d_pend};
            if (std::memcmp(&bufs_now, P.h_bufs, sizeof(DevBufs)) != 0) {
                *P.h_bufs = bufs_now;
                HIPCHK(hipMemcpyAsync(P.d_bufs, P.h_bufs, sizeof(DevBufs), hipMemcpyHostToDevice, P.stream));
            }
            // short conflict-free prefixes (a small array, colliding ops): the rounds of one persistent workgroup, no launch per round
            LAUNCH("burst", use_local ? launch_local_rounds(P.d_bufs, P.d_ctl, P.d_ops, P.d_rs, LOCAL_ROUNDS, pub, P.stream)
                                      : launch_burst(P.d_bufs, P.d_ctl, P.d_ops, P.d_rs, P.d_plans,
                                                     burst_rounds, burst_rounds == ROUNDS_PER_SYNC ? &P.burst : &P.burst_short, pub, P.stream));
        }
        wait_published(P);
        t_burst += elapsed_ms(tb0); ++n_burst;
        if (use_local) { t_local += elapsed_ms(tb0); ++n_local; r_local += rs.rounds; o_local += rs.par_ops; }
        // the prefix of the last round of the burst has been applied but is folded into the cursor only by the next round's resolve step
        if (rs.pad >= 10) fail(DSA_EASSERT, "DSA_FP_CHECK: a round of the batch-parallel writes is not equivalent to the sequential order (code " + std::to_string(rs.pad) + ", details on stdout)");
        if (rs.pad == 9) fail(DSA_EASSERT, "batch-parallel writes: a deferred op left the zone it was sealed in (internal invariant of the run-ahead rounds)");
        if (rs.pad != 0) fail(DSA_EASSERT, "batch-parallel column creation left its footprint (internal invariant)");
        // what the sequencer takes after a stop: the op that cannot be planned alone when the rounds were otherwise making progress
        // (the ops behind it are cheaper in a round: ~1 us each against 5-15 us), a chunk of SEQ_CHUNK0 ops when short prefixes
        // stopped them (the ops around the cursor collide); doubled while the rounds apply fewer than two ops each
        if (rs.par_ops >= 2 * std::max<int64_t>(1, rs.rounds)) seq_chunk = rs.why[7] > 0 ? SEQ_CHUNK0 : BARRIER_CHUNK0;
        // new partitions of the rounds sit at the end of the tables: back into key order with the whole chip once enough have piled up
        if (P.h_ctl->n_pending >= MERGE_AT) merge_tables(P);
        P.stat_par_rounds += rs.rounds; P.stat_par_ops += rs.par_ops; P.stat_deferred += rs.deferred;
        for (int q = 0; q < 8; ++q) P.stat_why[q] += rs.why[q];
        i = rs.cursor_n; np = rs.np_n; cur = rs.cur_n;
        G = rs.G; ema = rs.ema;
        burst_rounds = (rs.stop == 1 && rs.rounds <= ROUNDS_SHORT) ? ROUNDS_SHORT : ROUNDS_PER_SYNC;
        if (rs.stop == 5 || (drain && np == 0)) {          // the pending list is drained: what it was drained for
            drain = false;
            const int what = after_drain; after_drain = 0;
            if (what == 1) { use_local = true; continue; }
            if (what != 2) continue;
            to_sequencer = true;
        } else if (rs.stop == 1 && np > 0) {
            // the op at the head of the pending list cannot be planned (it needs the sequencer: a wide window, _extend!): everything in
            // front of it has been applied, so the sequencer takes exactly that op; then it leaves the list
            const int64_t op0 = rs.pend0;
            SeqRun r;
            r.P = &P; r.n = op0 + 1; r.n_avail = op0 + 1; r.active = true; r.defer_merge = true;
            P.h_ctl->next_op = op0; P.h_ctl->status = 0; P.h_ctl->err = 0; P.h_ctl->no_run_at = op0;       // (no append run from a pending op: the ops behind it are not its successors)
            seq_launch(r);
            while (seq_step(r)) ++n_yield;
            ++n_seq;
            if (r.err) fail(DSA_EASSERT, "batch-parallel writes: a deferred op failed in the sequencer (no op of a run-ahead batch can fail)");
            P.stat_seq_ops += 1; P.stat_seq_launches += 1;
            std::vector<PendOp> lst((size_t)np);
            HIPCHK(hipMemcpyAsync(lst.data(), P.d_pend + (size_t)cur * GMAX, (size_t)np * sizeof(PendOp), hipMemcpyDeviceToHost, P.stream));
            HIPCHK(hipStreamSynchronize(P.stream));
            if (lst[0].op != op0) fail(DSA_EASSERT, "batch-parallel writes: pending list out of step with the round state");
            --np;
            if (np > 0) { HIPCHK(hipMemcpyAsync(P.d_pend + (size_t)cur * GMAX, lst.data() + 1, (size_t)np * sizeof(PendOp), hipMemcpyHostToDevice, P.stream)); HIPCHK(hipStreamSynchronize(P.stream)); }
            continue;
        } else {
            bool want_local = false;
            if (use_local) { if (rs.stop == 3) { use_local = false; ema = 16 * 64; G = 64; } }   // full prefixes: the grid rounds pay again
            else if (local_ok && rs.rounds > 0 && ema < 16 * LOCAL_BELOW) want_local = true;     // prefixes of a few ops: one workgroup is enough
            // (the local rounds and the sequencer work on the contiguous rest of the batch: the pending list is drained first)
            if (want_local) { if (np > 0) { drain = true; after_drain = 1; continue; } use_local = true; }
            if (rs.stop != 1) continue;                       // burst used up (0), batch finished (2), or a switch of round kind (3)
            to_sequencer = true;
        }
        }
        if (!to_sequencer) continue;
        if (np > 0) { drain = true; after_drain = 2; continue; }
        seq_first = false;
        // ---- short prefix at op i: sequential sequencer for ops [i, i + seq_chunk)
        const auto ts0 = Clock::now();
        int64_t no_run_at = -1;
        for (;;) {
            SeqRun r;
            r.P = &P; r.n = std::min<int64_t>(n, i + seq_chunk); r.n_avail = n; r.active = true; r.defer_merge = true;
            P.h_ctl->next_op = i; P.h_ctl->status = 0; P.h_ctl->err = 0; P.h_ctl->no_run_at = no_run_at;
            const int64_t dbg_slots0 = P.h_ctl->stat_window_slots, dbg_reb0 = P.h_ctl->stat_rebalances, dbg_ext0 = P.h_ctl->stat_extends;
            seq_launch(r);
            while (seq_step(r)) ++n_yield;
            ++n_seq;
            if (r.err) { if (P.h_ctl->n_pending > 0) merge_tables(P); *err = r.err; return r.applied; }
            if (P.h_ctl->n_pending >= MERGE_AT) merge_tables(P);
            if (dbg_split && r.applied - i <= 2) {      // dev: what a one-op detour through the sequencer rebalanced (slots of its windows, log2 buckets)
                const int64_t ds = P.h_ctl->stat_window_slots - dbg_slots0;
                int b = 0; while ((1ll << b) < ds && b < 31) ++b;
                dbg_detour[P.h_ctl->stat_extends != dbg_ext0 ? 31 : b] += 1;
                (void)dbg_reb0;
            }
            P.stat_seq_ops += r.applied - i; P.stat_seq_launches += 1;
            i = r.applied;
            // an append run that stopped in front of op i (it needs _extend!): that op and what follows stay with the sequencer, which
            // detects the rest of the run behind it — no detour through a burst of rounds that cannot plan the op either
            if (i < n && P.h_ctl->no_run_at == i) { no_run_at = i; seq_chunk = std::max<int64_t>(seq_chunk, 8); continue; }
            break;
        }
        t_seq += elapsed_ms(ts0);
        seq_chunk = std::min<int64_t>(seq_chunk * 2, 8192);
        G = 64;
    }
    if (dbg_split)
        fprintf(stderr, "  [run_ops_parallel %s] n=%lld: %lld bursts %.2f ms (of which %lld local launches %.2f ms: %lld mini-rounds, %lld ops), %lld sequencer chunks (%lld yields) %.2f ms\n",
                P.has_cols ? "pcsc" : "vec", (long long)n, (long long)n_burst, t_burst, (long long)n_local, t_local, (long long)r_local, (long long)o_local,
                (long long)n_seq, (long long)n_yield, t_seq);
    if (dbg_split) {
        fprintf(stderr, "    one-op detours by window slots (log2 bucket: count; 31 = with _extend!):");
        for (int b = 0; b < 32; ++b) if (dbg_detour[b]) fprintf(stderr, " %d:%lld", b, (long long)dbg_detour[b]);
        fprintf(stderr, "\n");
        fprintf(stderr, "    sequencer chunks: waiting for the device %.2f ms; host work by yield kind [done %.2f, rebalance %.2f, extend %.2f, shrink %.2f, table %.2f, error %.2f, run %.2f] ms\n",
                g_seq_wait_ms, g_seq_host_ms[0], g_seq_host_ms[1], g_seq_host_ms[2], g_seq_host_ms[3], g_seq_host_ms[4], g_seq_host_ms[5], g_seq_host_ms[6]);
        fprintf(stderr, "    seq_launch calls %.2f ms\n", g_seq_launch_ms);
        g_seq_wait_ms = 0; g_seq_launch_ms = 0; for (double& x : g_seq_host_ms) x = 0;
    }
    if (P.h_ctl->n_pending > 0) merge_tables(P);          // the tables leave the batch in key order (the reference's numbering)
    return n;
}

// Two independent structures (the colmajor and rowmajor orientation): both sequencers run at the same time, each on
// its own stream; the host alternates between their yield mailboxes.
void run_ops_pair(Pma& A, const std::vector<Op>& opsA, Pma& B, const std::vector<Op>& opsB, SeqRun& ra, SeqRun& rb) {
    seq_start(ra, A, opsA);
    seq_start(rb, B, opsB);
    while (ra.active || rb.active) {
        if (ra.active) seq_step(ra);
        if (rb.active) seq_step(rb);
    }
}

}  // namespace host
}  // namespace dsa
