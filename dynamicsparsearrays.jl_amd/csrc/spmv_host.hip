// csrc/spmv_host.hip — the Pma-level half of the dense product, host side: what the gather launch may assume about an orientation
// (the SpmvMeta prefetch) and the cached column-swept plan (shape test, build, product, drop).  Host-only unit: kernels in spmv.hip.
#include "host.h"

#include <algorithm>
#include <chrono>
#include <cstring>

namespace dsa {
namespace host {

// What the gather launch may assume about an orientation (recomputed after every launch that can change the layout or
// the tables: one small kernel + an 8-byte round trip, amortised over the SpMV calls between two write batches).
// Tables with tombstones or unmerged entries take the memset path whatever the layout: nothing to compute.
static bool spmv_meta_applicable(const Pma& P) {
    const Ctl& c = *P.h_ctl;
    return P.has_cols && c.table_len > 0 && P.view().dense && c.n_pending == 0;
}
// Enqueues k_spmv_meta + the copy of its 5 result words behind whatever is on the stream (one launch, no host wait).  Called at the
// end of every write batch / build, so that the product that follows finds the words already in pinned memory: the product after a
// write batch costs what its kernel costs (round 2: a 359 us meta kernel + a host round trip in front of an 8.7 us SpMV in config 5).
void prefetch_spmv_meta(Pma& P) {
    if (P.spmv_meta.epoch == P.layout_epoch || P.meta_inflight_epoch == P.layout_epoch || !spmv_meta_applicable(P)) return;
    if (!P.d_meta) {
        HIPCHK(hipMalloc(&P.d_meta, SPMV_META_WORDS * sizeof(unsigned long long)));
        HIPCHK(hipMemsetAsync(P.d_meta, 0, SPMV_META_WORDS * sizeof(unsigned long long), P.stream));
        // words 0..5: k_spmv_meta's results + sequence number; 6..8: the SpMV plan build's (ok, cells, sequence number)
        HIPCHK(pinned_alloc(reinterpret_cast<void**>(&P.h_meta), 16 * sizeof(int64_t)));
        std::memset(P.h_meta, 0, 16 * sizeof(int64_t));
        P.meta_seq = 0;
    }
    // the kernel writes its five words and then the sequence number straight into pinned host memory
    LAUNCH("spmv meta", launch_spmv_meta(P.view(), P.d_meta,
                                         reinterpret_cast<unsigned long long*>(P.h_meta), ++P.meta_seq, P.stream));
    P.meta_inflight_epoch = P.layout_epoch;
}
const Pma::SpmvMeta& spmv_meta(Pma& P) {
    Pma::SpmvMeta& M = P.spmv_meta;
    if (M.epoch == P.layout_epoch) return M;
    M = Pma::SpmvMeta();
    M.epoch = P.layout_epoch;
    if (!spmv_meta_applicable(P)) return M;     // tombstones: memset path
    M.epoch = -1;
    prefetch_spmv_meta(P);                      // no-op when the write batch has already enqueued it
    // wait for the sequence number: normally there already (the kernel was enqueued behind the write batch); a stream wait if it
    // does not show up within a millisecond
    wait_policy_block(P);
    volatile int64_t* seqp = P.h_meta + 5;
    const auto t0 = std::chrono::steady_clock::now();
    bool synced = false;
    while ((unsigned long long)__atomic_load_n(seqp, __ATOMIC_ACQUIRE) != P.meta_seq) {
        if (!synced && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(1)) { HIPCHK(hipStreamSynchronize(P.stream)); synced = true; continue; }
        if (synced) fail(DSA_EHIP, "SpMV meta kernel finished without publishing its result");
    }
    M.epoch = P.layout_epoch;
    const int64_t* r = P.h_meta;
    M.ordered = r[4] == 0;
    M.max_extent = r[0]; M.max_gap = r[1]; M.first_key = r[2]; M.last_key = r[3];
    return M;
}

// ---- the column-swept plan (spmv.hip: k_spmv_plan) ----------------------------------------------------------------------------
// Taken by a dense product over the gather orientation when x does not fit an XCD's L2 (the gathers of k_spmv_gather miss there) and
// the ZFILL conditions hold (every row is written once).  Built on the SECOND product at one (content epoch, layout epoch, nx, ny) —
// a caller who writes between every two products never pays for it —, as three kernels on the product's stream; the build reports
// whether the plan is usable (rows per group within the LDS accumulators) through h_meta[6..8], read by the product after it.
bool spmv_plan_on() { static const bool on = [] { const char* e = dev_env("DSA_SPMV_PLAN"); return !(e && e[0] == '0'); }(); return on; }

// returns the plan's memory to the pool (after the work in flight on the stream that may still read it)
void spmv_plan_drop(Pma& P) {
    Pma::SpmvPlan& L = P.plan;
    if (L.mem[0] || L.mem[1]) {
        if (P.stream) (void)hipStreamSynchronize(P.stream);
        pool_free(L.mem[0]); pool_free(L.mem[1]);
    }
    const unsigned long long seq = L.seq;
    L = Pma::SpmvPlan();
    L.seq = seq;
}

static int plan_slices(int64_t nx) { return (int)std::max<int64_t>(16, (nx + 65535) / 65536); }

// (ny + 1 < 2^32: the plan's row map keeps the row keys clamped to [0, ny + 1] as 32-bit words)
bool spmv_plan_shape_ok(const Pma& P, int64_t nx, int64_t ny) {
    const int64_t groups = (P.capacity() + PLAN_GROUP_SLOTS - 1) / PLAN_GROUP_SLOTS;
    return groups <= PLAN_MAX_GROUPS && plan_slices(nx) <= PLAN_MAX_SLICES && P.h_ctl->nb_elements < ((int64_t)1 << 31) &&
           ny >= 0 && ny + 1 < ((int64_t)1 << 32);
}

void spmv_plan_build(Pma& P, int64_t nx, int64_t ny, hipStream_t s) {
    Pma::SpmvPlan& L = P.plan;
    PlanDev& d = L.dev;
    d.groups = (P.capacity() + PLAN_GROUP_SLOTS - 1) / PLAN_GROUP_SLOTS;
    d.slices = plan_slices(nx);
    d.width = (nx + d.slices - 1) / d.slices;
    d.cap_cells = std::max<int64_t>(1, P.h_ctl->nb_elements - P.h_ctl->table_len);      // every stored entry but the semaphores
    const int64_t G = d.groups, S = d.slices;
    const int64_t T = std::max<int64_t>(1, P.h_ctl->table_len);
    const int64_t words = G * (S + PLAN_DESC) + G * S + G + (G + 1) + G + T;                      // off, cnt, gbase, pfirst, nsem, yrow (uint32)
    HIPCHK(pool_alloc(&L.mem[0], (size_t)d.cap_cells * (sizeof(uint32_t) + sizeof(double))));
    HIPCHK(pool_alloc(&L.mem[1], (size_t)words * sizeof(uint32_t)));
    L.bytes = d.cap_cells * 12 + words * 4;
    d.val = static_cast<double*>(L.mem[0]);
    d.cell = reinterpret_cast<uint32_t*>(d.val + d.cap_cells);
    d.off = static_cast<uint32_t*>(L.mem[1]);
    d.cnt = d.off + G * (S + PLAN_DESC);
    d.gbase = d.cnt + G * S;
    d.pfirst = d.gbase + G;
    d.nsem = d.pfirst + G + 1;
    d.yrow = d.nsem + G;
    unsigned long long* out = reinterpret_cast<unsigned long long*>(P.h_meta + 6);
    launch_check(launch_spmv_plan_build(P.view(), nx, ny, d, out, ++L.seq, s), "spmv plan build: ");
    L.state = Pma::SpmvPlan::PENDING;
    ++P.stat_spmv_plan_builds;
}

// true when the product was computed from the plan; otherwise counts the product and builds the plan on the second one
bool spmv_plan_product(Pma& P, const double* d_x, int64_t nx, double* d_y, int64_t ny, hipStream_t s) {
    Pma::SpmvPlan& L = P.plan;
    if (L.content_epoch != P.content_epoch || L.layout_epoch != P.layout_epoch || L.nx != nx || L.ny != ny) {
        spmv_plan_drop(P);
        L.content_epoch = P.content_epoch; L.layout_epoch = P.layout_epoch; L.nx = nx; L.ny = ny;
    }
    ++L.products;
    if (L.state == Pma::SpmvPlan::PENDING) {
        HIPCHK(wait_pinned_seq(P.h_meta + 8, L.seq, s));
        const bool ok = __atomic_load_n(P.h_meta + 6, __ATOMIC_ACQUIRE) == 1;
        if (ok) L.state = Pma::SpmvPlan::USABLE;
        else {      // the rows of a group do not fit the accumulators: k_spmv_gather at this key from now on
            const int64_t ce = L.content_epoch, le = L.layout_epoch, pr = L.products;
            spmv_plan_drop(P);
            L.content_epoch = ce; L.layout_epoch = le; L.nx = nx; L.ny = ny; L.products = pr;
            L.state = Pma::SpmvPlan::UNUSABLE;
        }
    }
    if (L.state == Pma::SpmvPlan::USABLE) {
        LAUNCH("spmv plan", launch_spmv_plan(L.dev, P.h_ctl->table_len, d_x, d_y, ny, s));
        ++P.stat_spmv_plan;
        return true;
    }
    return false;
}

}  // namespace host
}  // namespace dsa
