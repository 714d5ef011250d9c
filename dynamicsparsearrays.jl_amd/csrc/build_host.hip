// csrc/build_host.hip — the bulk build (K-build) of one Pma, host side: one orientation from device-resident triples, both
// orientations of a matrix from one sort, the upload of the caller's arrays in front of them, and the events that order the emit +
// spread phases of concurrent builds.  Host-only unit: the sort / combine / emit kernels are in build.hip, the spread in rebalance.hip.
#include "host.h"

#include <algorithm>
#include <cstring>
#include <functional>
#include <mutex>

namespace dsa {
namespace host {

namespace {
// one pass over a key array the host is about to upload: value range (what K-build's composite needs), storage width, the reserved key
struct KeyScan {
    int64_t lo = INT64_MAX, hi = INT64_MIN; bool zero = false;
    void add(int64_t k) { lo = k < lo ? k : lo; hi = k > hi ? k : hi; zero = zero || k == 0; }
    void add(const int64_t* k, int64_t n) {
        int64_t l = lo, h = hi; bool z = zero;
        for (int64_t i = 0; i < n; ++i) { const int64_t v = k[i]; l = v < l ? v : l; h = v > h ? v : h; z |= v == 0; }
        lo = l; hi = h; zero = z;
    }
    bool empty() const { return hi < lo; }
    KeyRange range() const { KeyRange r; if (!empty()) { r.lo = lo; r.hi = hi; } return r; }
    bool fit32() const { return !needs_wide(range()); }
};

// Owns the scratch of one build (build.hip): whatever ends the scope — an exception of a sizing step, a failed launch — drains the
// build's stream and hands the block back (build_abort); release() is the same at the end of a build that went well.  A scratch that
// was never allocated, or that build.hip has already released on an error of its own, costs nothing here.
struct ScratchGuard {
    BuildScratch s;
    ScratchGuard() = default;
    ScratchGuard(const ScratchGuard&) = delete;
    ScratchGuard& operator=(const ScratchGuard&) = delete;
    ~ScratchGuard() { release(); }
    void release() { build_abort(s); }
};

// Sizes a structure that holds nothing it keeps for ncells cells in np partitions — tables, geometry, slot buffers, live flags, layout
// epoch, rebalance statistics — and returns the length of its cell stream (cells + semaphores).  Buffers that are large enough
// already (speculative ones, the small vector's upper bound) are kept.
int64_t size_fresh(Pma& P, int64_t ncells, int64_t np) {
    if (P.has_sems) {
        P.h_ctl->nb_partitions = np; P.h_ctl->table_len = np;
        ensure_tables(P, std::max<int64_t>(2 * np, 64));
    }
    const int64_t n = ncells + np;
    set_geometry_for_new(P, capacity_for(n), n);
    ensure_capacity_alloc(P, 2 * P.capacity());
    if (P.has_cols && np > 0) HIPCHK(hipMemsetAsync(P.col_live, 1, (size_t)np, P.stream));
    ++P.layout_epoch;
    P.h_ctl->stat_rebalances = 0; P.h_ctl->stat_window_slots = 0;
    if (P.capacity() != P.h_ctl->segment_capacity) { P.h_ctl->stat_rebalances = 1; P.h_ctl->stat_window_slots = P.capacity(); }
    return n;
}

// While the sort kernels run (build_prepare / build_derived_sort call `while_sorting` between enqueueing them and waiting for the
// counts): tables and slot buffers for the UPPER bounds — every triple a cell of its own, every partition of the key range present.
// The exact sizes are known only from the counts, but capacity_for is monotone and the allocations (13 of them, a dozen memsets) used
// to sit between the sort and the emit with the GPU idle: 180 of the 1500 us of config 3's closefillmode!.  Duplicates folded later
// only leave the buffers larger than needed (as after a _shrink!).  Only for a structure that holds nothing yet: growing an existing
// one waits for the stream (old contents are copied).
// BEST EFFORT: the upper bound can be far above what the counts will ask for (duplicate-heavy input: a fill buffer that overwrites
// the same cells, a vector fed repeated keys), so it is capped at a share of the memory that is free right now, an allocation that
// fails here is undone (the exact sizing of size_fresh gets its chance), and pma_build_dev hands buffers more than 4 x too large back
// once the counts are known.
int64_t partitions_ub(const KeyRange& pr, int64_t cells_ub) {      // partitions of at most cells_ub cells whose partition keys lie in pr
    return pr.known() ? std::min<int64_t>(cells_ub, (int64_t)std::min<uint64_t>((uint64_t)pr.hi - (uint64_t)pr.lo, (uint64_t)cells_ub) + 1) : cells_ub;
}
void release_prealloc(Pma& P) {
    (void)hipStreamSynchronize(P.stream);      // (the counts arrive through pinned memory: the memsets of the speculative blocks may still be queued)
    pma_free_buffers(P);
    P.cap_alloc = 0; P.occ_words = 0; P.occ_dirty[0] = P.occ_dirty[1] = 0;
    pool_free(P.sems); pool_free(P.col_keys); pool_free(P.col_live);
    P.sems = nullptr; P.col_keys = nullptr; P.col_live = nullptr; P.h_ctl->table_cap = 0;
}
// side (or nullptr: none): a stream that is idle at this moment; the memsets of the fresh blocks — tables, bitmaps: ~60 us per orientation —
// go there instead of queueing behind the sort on P's own stream, which waits for them through an event.  Returns whether P now holds
// speculative buffers.
bool prealloc_upper(Pma& P, int64_t cells_ub, int64_t np_ub, const hipStream_t* side) {
    if (P.cap_alloc != 0 || P.sems != nullptr) return false;
    const int64_t slots_ub = 2 * capacity_for(cells_ub + np_ub);
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); return false; }
    const double want = 2.0 * (double)slots_ub * (double)(P.kb() + sizeof(double)) + 68.0 * (double)np_ub;      // (68 = 4 x 17 bytes of tables per partition)
    if (want > 0.25 * ((double)free_b + (double)pool_idle_bytes())) return false;      // not speculatively: exact sizing after the counts
    try {
        {
            struct Swap { Pma& P; hipStream_t own; Swap(Pma& p, const hipStream_t* s) : P(p), own(p.stream) { if (s) P.stream = *s; }
                          ~Swap() { P.stream = own; } } sw(P, side);
            ensure_tables(P, std::max<int64_t>(2 * np_ub, 64));
            ensure_capacity_alloc(P, slots_ub);
        }
        if (side) {
            if (P.ev_handoff == nullptr) HIPCHK(hipEventCreateWithFlags(&P.ev_handoff, hipEventDisableTiming));
            HIPCHK(hipEventRecord(P.ev_handoff, *side));
            HIPCHK(hipStreamWaitEvent(P.stream, P.ev_handoff, 0));
        }
        return true;
    } catch (const Fail&) {
        (void)hipGetLastError();
        if (side) (void)hipStreamSynchronize(*side);
        release_prealloc(P);
        return false;
    }
}
}  // namespace

// ------------------------------------------------------------------------------------------------
// bulk builders (K-build): everything but the staging of the caller's arrays runs on the device
// ------------------------------------------------------------------------------------------------
// order of the emit + spread phases of concurrent K-builds on one device (see pma_build_dev)
constexpr int MAX_EMIT_DEVICES = 16;
static std::mutex g_emit_mu;
static hipEvent_t g_emit_done[MAX_EMIT_DEVICES] = {};
// K-build from device-resident triples: sort / combine / emit on the device (build.hip), then the full-array spread;
// semaphores[] positions are written by the spread kernel.
//   mode 0: one orientation of a matrix (MappedPackedCSC: partitions = distinct values of d_part)
//   mode 1: a vector (d_part == nullptr, no semaphores)         dynamicsparsevec  src/vector.jl:38-62
//   mode 2: PackedCSC with explicit partition ids 1..nparts      PackedCSC ctor    src/pcsr.jl:26-63
void pma_build_dev(Pma& P, const int64_t* d_part, const int64_t* d_key, const double* d_val, int64_t nnz, int32_t combine,
                   int mode, int64_t nparts_explicit, bool wide, KeyRange part_range, KeyRange key_range) {
    P.wide = wide;                     // decided by the caller from the host copy of the keys, before anything is allocated
    // fault injection for the error paths of the builders (tests): DSA_FAIL_BUILD=1 fails every build while it is set
    if (const char* fe = dev_env("DSA_FAIL_BUILD")) if (fe[0] == '1') fail(DSA_EHIP, "injected build failure (DSA_FAIL_BUILD)");
    if (nnz == 0) {
        std::vector<int64_t> ks; std::vector<double> vs;
        const int64_t np = mode == 2 ? nparts_explicit : 0;
        for (int64_t p = 1; p <= np; ++p) { ks.push_back(SEM_KEY); vs.push_back((double)p); }    // only semaphore cells
        if (P.has_sems) { P.h_ctl->nb_partitions = np; P.h_ctl->table_len = np; ensure_tables(P, std::max<int64_t>(2 * np, 64)); }
        build_from_packed(P, ks, vs);
        return;
    }
    ScratchGuard sc;          // (in front of the emit_order lock below: whatever throws unlocks first, then releases the scratch)
    int64_t counts[2] = {0, 0};
    const auto tp0 = Clock::now();
    bool prealloc_done = false;
    const std::function<void()> prealloc = [&] {
        const int64_t np_ub = mode == 0 ? partitions_ub(part_range, nnz) : (mode == 2 ? nparts_explicit : 0);
        prealloc_done = prealloc_upper(P, nnz, np_ub, nullptr);
    };
    const hipError_t e = build_prepare(d_part, d_key, d_val, nnz, part_range, key_range, sc.s, counts, P.stream, &prealloc);
    const auto tp1 = Clock::now();
    launch_check(e, "K-build prepare: ");
    const int64_t np = mode == 0 ? counts[1] : (mode == 2 ? nparts_explicit : 0);
    if (prealloc_done && P.cap_alloc > 8 * capacity_for(counts[0] + np) && P.cap_alloc > (1 << 20)) release_prealloc(P);
    const int64_t n = size_fresh(P, counts[0], np);
    const auto tp2 = Clock::now();
    // (the emit kernels are only enqueued: the spread goes in right behind them, the scratch of the sort is released after the one
    //  stream wait of upload_ctl instead of after a wait of its own)
    // The two orientations of a matrix are built side by side on two streams.  Their sort passes share the chip well; their emits — ten
    // million 8-byte gathers of the values by input index each — and spreads do not: 293 + 263 us side by side against 100 us each alone,
    // the spreads 118 + 78 against 54.  So the emit + spread of one build waits (on the device: an event, no host wait) for the emit +
    // spread of the build enqueued before it.
    std::unique_lock<std::mutex> emit_order(g_emit_mu);
    const bool ordered = P.device >= 0 && P.device < MAX_EMIT_DEVICES;      // (events belong to a device: one slot per device)
    if (ordered) {
        hipEvent_t& ev = g_emit_done[P.device];
        if (ev == nullptr) HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        else HIPCHK(hipStreamWaitEvent(P.stream, ev, 0));
    }
    launch_check(build_emit(d_val, combine, sc.s, P.K(), P.V(), P.has_cols ? P.col_keys : nullptr, mode, nparts_explicit, P.stream, false), "K-build emit: ");
    const auto tp3 = Clock::now();
    root_rebalance(P, n, P.capacity(), n, true);
    if (ordered) HIPCHK(hipEventRecord(g_emit_done[P.device], P.stream));
    emit_order.unlock();
    upload_ctl(P);
    sc.release();          // (stream already waited for: releases the scratch)
    if (dbg_time())
        fprintf(stderr, "  [pma_build_dev] prepare (alloc + sorts + scans) %.1f ms  tables/slot alloc %.1f ms  emit (+ free) %.1f ms  spread + ctl %.1f ms\n",
                elapsed_ms(tp0, tp1), elapsed_ms(tp1, tp2), elapsed_ms(tp2, tp3), elapsed_ms(tp3));
}

// Both orientations of a matrix from ONE sort of the caller's triples (round 6).  A = the orientation whose partitions are d_part
// (sorted as before: composite of (partition, key) + input index, values gathered at the emit); its emit also leaves the folded cells
// as composites of the TWIN B — partition bits and key bits swapped — which B's builder only has to sort by its partition bits
// (build_derived_*: 3 passes of 16-byte records instead of 5 passes + a composite pass, and no 10 M random gathers at its emit).
// B's sort runs on B's stream behind A's emit (an event) while A's spread is still running; A's slot buffers and tables are sized
// while A's sort runs, B's while B's (prealloc_upper: each on the OTHER orientation's stream, idle at that moment).  Returns false —
// with nothing done to B and A built as usual — when A's composite does not fit 64 bits (the general path of build.hip): the caller
// then builds B from the triples.
bool mat_build_both_dev(Pma& A, Pma& B, const int64_t* d_part, const int64_t* d_key, const double* d_val, int64_t nnz, bool wideA, bool wideB,
                        KeyRange part_range, KeyRange key_range) {
    A.wide = wideA; B.wide = wideB;
    ScratchGuard sa, sb;
    int64_t ca[2] = {0, 0}, cb[2] = {0, 0};
    try {
        const std::function<void()> pa = [&] { prealloc_upper(A, nnz, partitions_ub(part_range, nnz), &B.stream); };
        launch_check(build_prepare(d_part, d_key, d_val, nnz, part_range, key_range, sa.s, ca, A.stream, &pa), "K-build prepare: ");
        const bool derive = !sa.s.wide_path;
        const int64_t na = size_fresh(A, ca[0], ca[1]);
        if (derive)
            launch_check(build_derived_alloc(sb.s, ca[0], /*kbits*/ sa.s.pbits, /*pbits*/ sa.s.kbits, /*kmin*/ sa.s.pmin, /*pmin*/ sa.s.kmin, B.stream),
                         "K-build (twin) scratch: ");
        launch_check(build_emit(d_val, DSA_COMBINE_ADD, sa.s, A.K(), A.V(), A.col_keys, 0, 0, A.stream, false, derive ? sb.s.comp[0] : nullptr,
                                derive ? sb.s.val[0] : nullptr), "K-build emit: ");
        if (derive) {
            if (A.ev_handoff == nullptr) HIPCHK(hipEventCreateWithFlags(&A.ev_handoff, hipEventDisableTiming));
            HIPCHK(hipEventRecord(A.ev_handoff, A.stream));
            HIPCHK(hipStreamWaitEvent(B.stream, A.ev_handoff, 0));
        }
        root_rebalance(A, na, A.capacity(), na, true);
        if (derive) {
            // B: sort the cells A's emit left by B's partition bits (behind the event), flags, counts; B's partitions are A's keys
            const std::function<void()> pb = [&] { prealloc_upper(B, ca[0], partitions_ub(key_range, ca[0]), &A.stream); };
            launch_check(build_derived_sort(sb.s, cb, B.stream, &pb), "K-build (twin) sort: ");
            if (cb[0] != ca[0]) fail(DSA_EASSERT, "K-build: the twin orientation counts other cells than its sibling emitted");
            const int64_t nb = size_fresh(B, cb[0], cb[1]);
            launch_check(build_emit(nullptr, DSA_COMBINE_ADD, sb.s, B.K(), B.V(), B.col_keys, 0, 0, B.stream, false), "K-build (twin) emit: ");
            root_rebalance(B, nb, B.capacity(), nb, true);
        }
        upload_ctl(A);                   // (waits for A's stream: its scratch is free)
        sa.release();
        if (derive) { upload_ctl(B); sb.release(); }
        return derive;
    } catch (...) {
        // emit and sort kernels may still run on either stream: they read the scratch the guards release behind this handler and the
        // caller's triples, which are the caller's again as soon as this throws
        (void)hipStreamSynchronize(A.stream); (void)hipStreamSynchronize(B.stream);
        throw;
    }
}

// uploads host arrays (any of them may be nullptr) and runs the device builder
void pma_build_from_host(Pma& P, const int64_t* part, const int64_t* key, const double* val, int64_t nnz, int32_t combine,
                         int mode, int64_t nparts_explicit) {
    if (mode == 1 && part == nullptr && nnz >= 1 && nnz <= VIEW_AREA_CELLS && dev_env("DSA_FAIL_BUILD") == nullptr) {
        // a small vector: ONE launch sorts, folds and packs the caller's pairs (read from the pinned landing area) in front of the slot
        // buffers and hands the entry count back; then the spread (the general builder: 130 us for 50 entries, this path ~45)
        KeyScan ks; ks.add(key, nnz);
        P.wide = !ks.fit32();
        ViewAreaLease lease(P);
        std::memcpy(P.h_view + 8, key, (size_t)nnz * sizeof(int64_t));
        std::memcpy(P.h_view + 8 + VIEW_AREA_CELLS, val, (size_t)nnz * sizeof(double));
        ensure_capacity_alloc(P, 2 * capacity_for(nnz));          // (an upper bound: folding can only shorten the stream)
        const unsigned long long seq = ++P.view_seq;
        __atomic_thread_fence(__ATOMIC_RELEASE);
        LAUNCH("small build", launch_build_small_vec(P.h_view, (int)nnz, (int)VIEW_AREA_CELLS, combine, P.K(), P.V(), seq, P.stream));
        wait_handover(P, P.h_view + 5, seq, "small build");
        const int64_t n = P.h_view[0];
        if (n < 1 || n > nnz) fail(DSA_EASSERT, "small build returned an impossible entry count");
        size_fresh(P, n, 0);             // (geometry for the n entries; the buffers above are large enough)
        root_rebalance(P, n, P.capacity(), n, true);
        upload_ctl(P);
        return;
    }
    int64_t *dP = nullptr, *dK = nullptr; double* dV = nullptr;
    auto release = [&] { pool_free(dP); pool_free(dK); pool_free(dV); };
    try {
        if (nnz > 0) {
            if (part) { HIPCHK(pool_alloc(reinterpret_cast<void**>(&dP), (size_t)nnz * 8)); HIPCHK(hipMemcpyAsync(dP, part, (size_t)nnz * 8, hipMemcpyHostToDevice, P.stream)); }
            HIPCHK(pool_alloc(reinterpret_cast<void**>(&dK), (size_t)nnz * 8)); HIPCHK(hipMemcpyAsync(dK, key, (size_t)nnz * 8, hipMemcpyHostToDevice, P.stream));
            HIPCHK(pool_alloc(reinterpret_cast<void**>(&dV), (size_t)nnz * 8)); HIPCHK(hipMemcpyAsync(dV, val, (size_t)nnz * 8, hipMemcpyHostToDevice, P.stream));
            HIPCHK(hipStreamSynchronize(P.stream));
        }
        KeyScan ks; ks.add(key, nnz);                        // (runs while the uploads above are in flight when they are asynchronous)
        KeyRange pr;
        if (part && mode == 2) { pr.lo = 1; pr.hi = std::max<int64_t>(nparts_explicit, 1); }
        pma_build_dev(P, dP, dK, dV, nnz, combine, mode, nparts_explicit, !ks.fit32(), pr, ks.range());
    } catch (...) {
        (void)hipStreamSynchronize(P.stream);
        release();
        throw;
    }
    release();
}

}  // namespace host
}  // namespace dsa
