// csrc/dsa_host.hip — the handle layer of libdsa_hip.so: the last-error text, the roctx loader, the table of development switches,
// what is written in terms of dsa_vec / dsa_pcsc (flush and apply of queued vector writes, packs, slices), the dense product of a
// matrix, and the C ABI of include/dsa.h.
//
// The matrix entry points are short wrappers: the argument checks that belong to the ABI plus one or two calls.  What they call is in
// units of its own: the fill-mode buffer in fill_host.hip, every write to a matrix (the builds of both orientations, the set batch
// and its strategies, the flush of queued writes, the delete of one column or row) in matwrite_host.hip; the exports, the products,
// the device import and the reductions in export_host.hip, spmm_host.hip, selprod_host.hip, spgemm_host.hip, ingest_host.hip and
// scale_host.hip; the in-place mutators (scale, batched delete, droptol, update, insert), the sparse-x product, the vector as a device
// operand and the parity hooks have entry points of their own in mutate_host.hip, sparsex_host.hip, vecops_host.hip and raw_host.hip.
// Everything that works on ONE packed-memory array (the Pma of host.h) is in the engine units pma_host.hip (lifecycle, geometry,
// rebalances, reads), writes_host.hip (yield loop around the sequencer, batch-parallel rounds), build_host.hip (K-build) and
// spmv_host.hip (SpMV meta and plan).
//
// Everything that touches slots runs on the GPU (rebalance.hip, sequencer.hip, spmv.hip).  The host
// keeps only: the control scalars of each PMA (mirrored from the device control block), the integer
// density bounds derived from the reference's Float64 thresholds (src/pma.jl:58,70,87 and :120-121),
// and the fill-mode staging buffer (src/buffer.jl — a host Dict in the reference as well).  The bulk builder
// (sort by (col,row), combine, emit, spread) runs on the device (build.hip + rebalance.hip).
// There is no CPU fallback for any slot operation.
#include "host.h"

#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace dsa;
using namespace dsa::host;

namespace {
thread_local std::string g_err;
}  // namespace

// roctx ranges around every ABI entry point (tracing): DSA_ROCTX=1 binds librocprofiler-sdk-roctx.so (or the legacy
// libroctx64.so) at run time, and `rocprofv3 --marker-trace` then shows which call a kernel belongs to; without the knob the
// cost is one predictable branch per call and no profiler library is mapped.
namespace dsa {
namespace host {
Roctx::Roctx() {
    const char* e = getenv("DSA_ROCTX");
    if (!(e && e[0] == '1')) return;
    for (const char* n : {"librocprofiler-sdk-roctx.so.1", "librocprofiler-sdk-roctx.so", "libroctx64.so.4", "libroctx64.so"}) {
        void* lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
        if (!lib) continue;
        push = reinterpret_cast<int (*)(const char*)>(dlsym(lib, "roctxRangePushA"));
        pop = reinterpret_cast<int (*)()>(dlsym(lib, "roctxRangePop"));
        if (push && pop) return;
        push = nullptr; pop = nullptr;
    }
}
const Roctx& roctx() { static const Roctx r; return r; }
}  // namespace host
}  // namespace dsa

// ---- the one table of development switches (dsa_dev.h: dev_env) --------------------------------------------------------------------
namespace dsa {
static const char* const k_dev_switches[] = {
    "DSA_BUILD_WIDE",     // 1: K-build through the general (> 64-bit composite) path
    "DSA_COUNT_MODEL",    // 0: bitmap-only append replay (no model v2)
    "DSA_DBG_RUN", "DSA_DBG_SPLIT", "DSA_DBG_TIME",      // timing / trace prints
    "DSA_DBG_MOVE2",      // ablations of the rebalance kernel (wrong results, timed)
    "DSA_FAIL_BUILD",     // 1: fails the next bulk build (fault injection, tests)
    "DSA_FP_MODE",        // footprint-check build (-DDSA_FP_CHECK): 1 recorded read / write sets, 2 sequential shadow re-plan (parbatch.hip)
    "DSA_KEYS_WIDE",      // 1: 64-bit physical keys everywhere
    "DSA_LOCAL_ROUNDS",   // 0: no local rounds (grid rounds only)
    "DSA_MODEL3",         // 0: no count-only append replay
    "DSA_MODEL5",         // 0: no typed multi-level replay of 8-slot-segment append runs
    "DSA_PARBATCH",       // 0: no batch-parallel rounds
    "DSA_POS_WIDE",       // 1: 64-bit positions in the append replay
    "DSA_RUN_AHEAD",      // 0: the rounds apply the conflict-free PREFIX only (rounds 2-5)
    "DSA_SPMV_PLAN",      // 0: never build or use the column-swept SpMV plan
    "DSA_SPMV_SHARE", "DSA_SPMV_STREAM",      // variants of the gather kernel
    "DSA_SPX_XDRIVEN",    // 0 / 1: the sparse-x product always through the gather kernel / always driven by x's entries
    "DSA_TIGHT",          // 0..3: tight footprints of leaf-accepted ops
};
const char* dev_env(const char* name) {
#ifndef NDEBUG
    bool known = false;
    for (const char* s : k_dev_switches) known = known || std::strcmp(s, name) == 0;
    if (!known) { fprintf(stderr, "dev_env: %s is not in the table of development switches\n", name); abort(); }
#endif
#ifndef DSA_DEV
    const char* on = getenv("DSA_DEV");
    if (!(on && on[0] == '1')) return nullptr;
#endif
    return getenv(name);
}

hipError_t wait_pinned_seq(const volatile void* word, uint64_t want, hipStream_t s, uint64_t mask) {
    const volatile unsigned long long* w = static_cast<const volatile unsigned long long*>(word);
    auto published = [&] { return (__atomic_load_n(w, __ATOMIC_ACQUIRE) & mask) == want; };
    auto next_query = std::chrono::steady_clock::now() + std::chrono::milliseconds(2);
    while (!published()) {
        if (std::chrono::steady_clock::now() < next_query) continue;
        const hipError_t q = hipStreamQuery(s);
        if (q == hipErrorNotReady) { next_query = std::chrono::steady_clock::now() + std::chrono::milliseconds(2); continue; }
        if (q != hipSuccess) return q;
        if (!published()) return hipErrorUnknown;
    }
    return hipSuccess;
}
void set_last_error(const char* msg) { g_err = msg ? msg : ""; }
}  // namespace dsa

// ------------------------------------------------------------------------------------------------
// handles (the structs are in host.h)
// ------------------------------------------------------------------------------------------------
namespace {

// Single setindex! calls are write-combined on the host (the "buffered batched writes" of the path): they are queued and
// applied, in order, by ONE sequencer launch at the latest before the next call that observes the structure.
constexpr size_t PENDING_FLUSH = 1u << 16;

Pma& orient(dsa_mat* h, int32_t o) {
    if (!h->has_major) fail(DSA_EMODE, "matrix is in fill mode");
    if (o != DSA_COLMAJOR && o != DSA_ROWMAJOR) fail(DSA_EARG, "orientation must be 0 or 1");
    return o == DSA_COLMAJOR ? h->col : h->row;
}

void vec_apply(dsa_vec_t* h, const int64_t* keys, const double* vals, int64_t n) {
    int32_t err = 0;
    static const bool par = [] { const char* e = dev_env("DSA_PARBATCH"); return !(e && e[0] == '0'); }();
    int64_t done;
    if (par && n >= 128) done = run_ops_parallel(h->P, OpBatch(OP_VEC_SET, keys, nullptr, vals, n), &err);      // the caller's columns go up as they are
    else {
        std::vector<Op> ops((size_t)n);
        for (int64_t i = 0; i < n; ++i) ops[(size_t)i] = make_op(OP_VEC_SET, keys[i], 0, vals[i]);
        done = run_ops(h->P, ops, &err);
    }
    const int64_t upto = err ? std::min(done + 1, n) : done;          // v.n is updated before the write (src/vector.jl:77-79)
    for (int64_t i = 0; i < upto; ++i) if (vals[i] != 0.0) h->n = std::max(h->n, keys[i]);
    if (err) fail(err, err_text(err));
}
// PackedMemoryArray(elements) (src/pma.jl:69-84) of the n cells packed at the front of S's alternate buffer (view_dev: ascending,
// distinct keys — nothing to sort or fold): geometry on the host, then ONE k_move2<PACKED> from S's buffer straight into the new
// vector's slot array.  The cells never leave HBM.  Everything is enqueued on S's stream (the pack that produced the cells runs
// there); the new vector gets its own stream back before it is handed out, after the one wait of upload_ctl.
dsa_vec* vec_from_packed_dev(Pma& S, int64_t n, int64_t len) {
    auto* v = new dsa_vec();
    hipStream_t own = nullptr;
    try {
        pma_init_common(v->P, false, false);
        Pma& P = v->P;
        own = P.stream; P.stream = S.stream;
        P.wide = S.wide;
        const int64_t capacity = capacity_for(n);
        set_geometry_for_new(P, capacity, n);
        ensure_capacity_alloc(P, 2 * capacity, false);
        ++P.layout_epoch; ++P.stat_grid_rebalances;
        P.h_ctl->stat_rebalances = 0; P.h_ctl->stat_window_slots = 0;
        if (capacity != P.h_ctl->segment_capacity) { P.h_ctl->stat_rebalances = 1; P.h_ctl->stat_window_slots = capacity; }
        // TWO launches make the vector: (1) both bitmaps, the status table of the grid rebalance and the control block (passed by value:
        // no copy command, the pinned mirror is not a DMA source) — five stream commands and a wait until round 6; (2) the spread
        LAUNCH("init", launch_init_fresh(P.occ[0], P.occ[1], P.occ_words, P.work.status, P.work.status_cap, P.d_ctl, *P.h_ctl, P.stream));
        const int salt = 1 - S.cur;
        // (root_rebalance of P with a foreign source: cells of S.alt[1..n] -> P.cur[1..capacity])
        LAUNCH("rebalance", launch_rebalance(S.KA(salt), S.vals[salt], S.occ[salt], 1, n, true, P.K(), P.V(), P.O(), 1, capacity, n,
                                             nullptr, &P.work, P.stream));
        P.occ_dirty[P.cur] = (capacity + 63) / 64;
        // the vector's own stream waits (on the device) for what was enqueued on S's; whatever S does next with its alternate buffer is
        // stream-ordered behind the spread.  No host wait.
        if (S.ev_handoff == nullptr) HIPCHK(hipEventCreateWithFlags(&S.ev_handoff, hipEventDisableTiming));
        HIPCHK(hipEventRecord(S.ev_handoff, S.stream));
        HIPCHK(hipStreamWaitEvent(own, S.ev_handoff, 0));
        P.stream = own;
    } catch (...) {
        if (own) { (void)hipStreamSynchronize(v->P.stream); v->P.stream = own; }
        pma_destroy(v->P); delete v; throw;
    }
    v->n = len;
    return v;
}

}  // namespace

// what sparsex_host.hip and vecops_host.hip call as well (declared in host.h)
namespace dsa {
namespace host {

void vec_flush(dsa_vec_t* h) {
    bind_device(h->P);
    if (h->pk.empty()) return;
    std::vector<int64_t> k; std::vector<double> v;
    k.swap(h->pk); v.swap(h->pv);                      // the queue is empty even if the apply fails
    vec_apply(h, k.data(), v.data(), (int64_t)k.size());
}

// K-pack of the whole vector into its alternate slot buffer (free between rebalances); returns the number of stored cells.
// The count is known on return, the packed cells are still being written on the vector's OWN stream: a consumer on another stream
// (the other operand of == / +) must wait for it (wait_for_pack).
int64_t vec_pack_alt(dsa_vec_t* h) {
    Pma& P = h->P;
    int64_t cnt = 0;
    const int alt = 1 - P.cur;
    {
        const int64_t c = pack_small(P, P.K(), P.V(), P.O(), 1, P.capacity(), P.KA(alt), P.vals[alt], P.cap_alloc);
        if (c >= 0) return c;
    }
    LAUNCH("compact", launch_compact_range(P.K(), P.V(), P.O(), 1, P.capacity(), P.KA(alt), P.vals[alt], P.cap_alloc, &P.work, &cnt, P.stream));
    return cnt;
}
// the packed cells of `producer` (vec_pack_alt) are complete before anything enqueued on `consumer`'s stream afterwards runs
void wait_for_pack(dsa_vec_t* producer, dsa_vec_t* consumer) {
    if (producer->P.stream == consumer->P.stream) return;
    HIPCHK(hipStreamSynchronize(producer->P.stream));
}

void ensure_xy(dsa_mat* h, int64_t nx, int64_t ny) {
    if (nx > h->x_cap) { if (h->d_x) hipFree(h->d_x); h->x_cap = std::max<int64_t>(nx, 1024); HIPCHK(hipMalloc(&h->d_x, (size_t)h->x_cap * sizeof(double))); }
    if (ny > h->y_cap) { if (h->d_y) hipFree(h->d_y); h->y_cap = std::max<int64_t>(ny, 1024); HIPCHK(hipMalloc(&h->d_y, (size_t)h->y_cap * sizeof(double))); }
}

// mat * v walks the colmajor orientation in the reference (src/operations.jl:14-24), transpose(mat) * v the
// rowmajor one (:26-36).  Gather form: the twin orientation, whose partitions are the OUTPUT index.
void spmv_dev(dsa_mat* h, int32_t transpose, int32_t algo, const double* d_x, int64_t nx, double* d_y, int64_t ny, hipStream_t s,
              int pattern) {
    if (!h->has_major) fail(DSA_EMODE, "matrix is in fill mode");
    hipError_t e;
    if (algo == 0) {
        Pma& P = transpose ? h->col : h->row;
        int mode = 0;
        // no memset of y when every row is written exactly once by the kernel: no partition longer than a span (no atomics)
        // and the rows without a partition are few (the owner of the next partition zeroes them)
        constexpr int64_t MAX_FILL = 4096;
        const Pma::SpmvMeta& M = spmv_meta(P);
        if (M.ordered && M.max_extent <= SPMV_SPAN_SLOTS && M.max_gap <= MAX_FILL && M.first_key >= 1 && M.first_key <= MAX_FILL &&
            ny - M.last_key <= MAX_FILL)
            { mode |= SPMV_ZFILL; ++P.stat_spmv_nomemset; }
        if (nx * (int64_t)sizeof(double) <= (3 << 20)) mode |= SPMV_PLAIN_STREAM;      // x stays in an XCD's 4 MB L2 beside the stream
        const bool plan = spmv_plan_on() && pattern == 0 && (mode & SPMV_ZFILL) && !(mode & SPMV_PLAIN_STREAM) && s == P.stream &&
                          nx > 0 && spmv_plan_shape_ok(P, nx, ny);
        if (plan && spmv_plan_product(P, d_x, nx, d_y, ny, s)) return;
        e = launch_spmv_gather(P.view(), d_x, nx, d_y, ny, pattern, mode, s);
        if (e == hipSuccess && plan && P.plan.state == Pma::SpmvPlan::NONE && P.plan.products == 2) spmv_plan_build(P, nx, ny, s);
    } else if (algo == 1) {
        Pma& P = transpose ? h->row : h->col;
        e = launch_spmv_scatter(P.view(), d_x, nx, d_y, ny, s);
    } else {
        fail(DSA_EARG, "algo must be 0 (gather) or 1 (scatter)");
    }
    launch_check(e, "spmv launch: ");
}

}  // namespace host
}  // namespace dsa

namespace {

void _check_status(int32_t rc) { if (rc != DSA_OK) fail(rc, g_err); }

int32_t view_impl(dsa_mat_t* h, int32_t o, int64_t key, int64_t* ks, double* vs, int64_t cap, int64_t* n_out) {
    API_TRY
    mat_flush(h);
    if (h->fillmode) fail(DSA_EMODE, "View not available in fill mode.");
    std::vector<int64_t> k; std::vector<double> v;
    col_view_of(orient(h, o), key, k, v);
    if ((int64_t)k.size() > cap) fail(DSA_ECAP, "output buffers too small");
    std::copy(k.begin(), k.end(), ks); std::copy(v.begin(), v.end(), vs);
    *n_out = (int64_t)k.size();
    API_CATCH
}

// m[:, col] (src/pcsr.jl:285-291 -> :247-259) and m[row, :] (src/pcsr.jl:269-283; served from the rowmajor twin, whose
// partition `row` holds exactly the (col, value) pairs the reference collects by scanning the colmajor array)
int32_t slice_impl(dsa_mat_t* h, int32_t o, int64_t key, dsa_vec_t** out) {
    API_TRY
    mat_flush(h);
    if (h->fillmode) fail(DSA_EMODE, "slices are not available in fill mode");
    Pma& S = orient(h, o);
    const auto ts0 = Clock::now();
    const DevView dv = view_dev(S, key);
    const auto ts1 = Clock::now();
    if (dv.cnt <= 0) { _check_status(dsa_vec_create(nullptr, nullptr, 0, DSA_COMBINE_ADD, 0, out)); return DSA_OK; }      // PackedMemoryArray(L, T)  src/pcsr.jl:288
    *out = vec_from_packed_dev(S, dv.cnt, std::max<int64_t>(dv.last_key, 0));          // _guess_length(pma)  src/vector.jl:7-8
    if (dbg_time()) fprintf(stderr, "[slice] %lld cells: view %.1f us, new vector %.1f us\n", (long long)dv.cnt, elapsed_us(ts0, ts1), elapsed_us(ts1));
    API_CATCH
}
// @view m[:, col] / @view m[row, :] with the cells delivered into HBM: d_keys / d_vals are DEVICE arrays of `cap` entries; the copy is
// enqueued on the orientation's stream (dsa_mat_set_stream / dsa_mat_sync), the count is known on return
int32_t view_dev_impl(dsa_mat_t* h, int32_t o, int64_t key, int64_t* d_keys, double* d_vals, int64_t cap, int64_t* n_out) {
    API_TRY
    mat_flush(h);
    if (h->fillmode) fail(DSA_EMODE, "View not available in fill mode.");
    Pma& S = orient(h, o);
    const DevView dv = view_dev(S, key);
    *n_out = 0;
    if (dv.cnt <= 0) return DSA_OK;
    if (dv.cnt > cap) fail(DSA_ECAP, "output buffers too small");
    const int salt = 1 - S.cur;
    if (S.wide) HIPCHK(hipMemcpyAsync(d_keys, S.keys[salt], (size_t)dv.cnt * sizeof(int64_t), hipMemcpyDeviceToDevice, S.stream));
    else {
        launch_check(launch_widen_keys(S.keys[salt], d_keys, dv.cnt, S.stream), "view copy-out: ");
    }
    HIPCHK(hipMemcpyAsync(d_vals, S.vals[salt], (size_t)dv.cnt * sizeof(double), hipMemcpyDeviceToDevice, S.stream));
    *n_out = dv.cnt;
    API_CATCH
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
extern "C" {

const char* dsa_last_error_message(void) { return g_err.c_str(); }

int32_t dsa_device_count(int32_t* count) {
    API_TRY
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *count = 0; fail(DSA_EHIP, std::string("hipGetDeviceCount: ") + hipGetErrorString(e)); }
    *count = n;
    API_CATCH
}
// the caching allocator (pool.hip) keeps up to DSA_POOL_MAX_MB of idle HBM per process: a host that shares the card with another
// allocator (PyTorch's) asks how much that is and hands it back
int32_t dsa_pool_idle_bytes(int64_t* bytes) { API_TRY *bytes = (int64_t)pool_idle_bytes(); API_CATCH }
int32_t dsa_pool_trim(int64_t keep_bytes) { API_TRY pool_trim(keep_bytes > 0 ? (size_t)keep_bytes : 0); API_CATCH }
int32_t dsa_dev_switches(char* buf, int64_t cap, int32_t* enabled) {
    API_TRY
    std::string all;
    for (const char* s : dsa::k_dev_switches) { if (!all.empty()) all += ' '; all += s; }
    if (buf == nullptr || cap < (int64_t)all.size() + 1) fail(DSA_ECAP, "buffer too small for the list of development switches");
    std::memcpy(buf, all.c_str(), all.size() + 1);
    if (enabled) {
#ifdef DSA_DEV
        *enabled = 1;
#else
        const char* on = getenv("DSA_DEV");
        *enabled = (on && on[0] == '1') ? 1 : 0;
#endif
    }
    API_CATCH
}
int32_t dsa_set_device(int32_t device) {
    API_TRY
    HIPCHK(hipSetDevice(device));
    g_device = device;
    API_CATCH
}

}  // extern "C"

extern "C" {

// ---------------- vector ----------------
int32_t dsa_vec_create(const int64_t* keys, const double* vals, int64_t n, int32_t combine_op, int64_t len, dsa_vec_t** out) {
    API_TRY
    if (n < 0) fail(DSA_EARG, "negative length");
    if (len < 0) { len = 0; for (int64_t i = 0; i < n; ++i) len = std::max(len, keys[i]); }      // _guess_length  src/vector.jl:6
    if (n > 0xffffffffll) fail(DSA_EARG, "more than 2^32-1 entries in one call");
    auto* h = new dsa_vec();
    try {
        pma_init_common(h->P, false, false);
        // _prepare_keys_vals! (stable sort + left fold of duplicates, src/vector.jl:10-36) and the spread, on the device
        pma_build_from_host(h->P, nullptr, keys, vals, n, combine_op, 1, 0);
    } catch (...) { pma_destroy(h->P); delete h; throw; }
    h->n = len;
    *out = h;
    API_CATCH
}
int32_t dsa_vec_create_empty(dsa_vec_t** out) { return dsa_vec_create(nullptr, nullptr, 0, DSA_COMBINE_ADD, -1, out); }
int32_t dsa_vec_destroy(dsa_vec_t* h) { if (h) { pma_destroy(h->P); delete h; } return DSA_OK; }

int32_t dsa_vec_get_batch(dsa_vec_t* h, const int64_t* keys, int64_t n, double* out) {
    API_TRY vec_flush(h); get_batch(h->P, 0, keys, nullptr, n, out); API_CATCH
}
int32_t dsa_vec_get(dsa_vec_t* h, int64_t key, double* out) { return dsa_vec_get_batch(h, &key, 1, out); }

int32_t dsa_vec_set_batch(dsa_vec_t* h, const int64_t* keys, const double* vals, int64_t n) {
    API_TRY
    vec_flush(h);
    vec_apply(h, keys, vals, n);
    API_CATCH
}
int32_t dsa_vec_set(dsa_vec_t* h, int64_t key, double val) {      // queued; see PENDING_FLUSH
    API_TRY
    if (val != 0.0) h->n = std::max(h->n, key);
    h->pk.push_back(key); h->pv.push_back(val);
    if (h->pk.size() >= PENDING_FLUSH) vec_flush(h);
    API_CATCH
}
int32_t dsa_vec_nnz(dsa_vec_t* h, int64_t* out) { API_TRY vec_flush(h); *out = h->P.h_ctl->nb_elements; API_CATCH }
int32_t dsa_vec_len(dsa_vec_t* h, int64_t* out) { *out = h->n; return DSA_OK; }

int32_t dsa_vec_nonzeros(dsa_vec_t* h, int64_t* keys, double* vals, int64_t cap, int64_t* n_out) {
    API_TRY
    vec_flush(h);
    std::vector<int64_t> ks; std::vector<double> vs;
    read_range(h->P, 1, h->P.capacity(), ks, vs);
    if ((int64_t)ks.size() > cap) fail(DSA_ECAP, "output buffers too small");
    std::copy(ks.begin(), ks.end(), keys); std::copy(vs.begin(), vs.end(), vals);
    *n_out = (int64_t)ks.size();
    API_CATCH
}
// v1 == v2  src/vector.jl:85-87 (lengths, then src/pma.jl:262-266: nb_elements, then the stored tuples pairwise in slot order,
// _arrays_equal src/pma.jl:236-260); compared on the device, only the verdict crosses PCIe
int32_t dsa_vec_equal(dsa_vec_t* a, dsa_vec_t* b, int32_t* out) {
    API_TRY
    vec_flush(a);
    if (a == b) { *out = 1; return DSA_OK; }
    vec_flush(b);
    *out = 0;
    if (a->n != b->n || a->P.h_ctl->nb_elements != b->P.h_ctl->nb_elements) return DSA_OK;
    const int64_t n = a->P.h_ctl->nb_elements;
    if (n == 0) { *out = 1; return DSA_OK; }
    if (vec_pack_alt(a) != n || vec_pack_alt(b) != n) fail(DSA_EASSERT, "stored-cell count differs from nb_elements");
    Pma &A = a->P, &B = b->P;
    wait_for_pack(b, a);
    HIPCHK(hipMemsetAsync(A.d_err, 0, sizeof(int32_t), A.stream));
    LAUNCH("compare", launch_packed_equal(A.KA(1 - A.cur), A.vals[1 - A.cur], B.KA(1 - B.cur), B.vals[1 - B.cur], n, A.d_err, A.stream));
    int32_t differ = 0;
    HIPCHK(hipMemcpyAsync(&differ, A.d_err, sizeof(int32_t), hipMemcpyDeviceToHost, A.stream));
    HIPCHK(hipStreamSynchronize(A.stream));
    *out = differ ? 0 : 1;
    API_CATCH
}
// alpha * a + beta * b as ascending (key, value) pairs — the SparseVector the reference's v1 + v2 / v1 - v2 / -v evaluate to
// through the AbstractSparseVector fallbacks over nonzeroinds / nonzeros (src/vector.jl:93-109; test/functional/math.jl:53-94).
// Both operands are packed and merged on the device; a key stored in both keeps one entry unless its value is zero.
int32_t dsa_vec_axpby(dsa_vec_t* a, double alpha, dsa_vec_t* b, double beta, int64_t* keys, double* vals, int64_t cap, int64_t* n_out) {
    API_TRY
    vec_flush(a);
    if (b != a) vec_flush(b);
    *n_out = 0;
    const int64_t na = vec_pack_alt(a);
    const int64_t nb = b != a ? vec_pack_alt(b) : na;
    const int64_t total = na + nb;
    if (total == 0) return DSA_OK;
    Pma &A = a->P, &B = b->P;
    if (b != a) wait_for_pack(b, a);
    const int64_t nwords = (total + 63) >> 6, ntiles = (nwords + 63) / 64;
    char* scratch = nullptr;
    const size_t off_mv = (size_t)total * 8, off_ok = 2 * off_mv, off_ov = 3 * off_mv, off_keep = 4 * off_mv,
                 off_cnt = off_keep + (size_t)nwords * 8, off_off = off_cnt + (size_t)(ntiles + 8) * 4, bytes = off_off + (size_t)(ntiles + 8) * 4;
    HIPCHK(pool_alloc(reinterpret_cast<void**>(&scratch), bytes));      // (the caching allocator: a hipMalloc + hipFree pair per call cost more than the kernels)
    try {
        int64_t* mk = reinterpret_cast<int64_t*>(scratch);
        double* mv = reinterpret_cast<double*>(scratch + off_mv);
        int64_t* ok = reinterpret_cast<int64_t*>(scratch + off_ok);
        double* ov = reinterpret_cast<double*>(scratch + off_ov);
        uint64_t* keep = reinterpret_cast<uint64_t*>(scratch + off_keep);
        RebalanceWork work{reinterpret_cast<uint32_t*>(scratch + off_cnt), reinterpret_cast<uint32_t*>(scratch + off_off), ntiles + 8};
        HIPCHK(hipMemsetAsync(keep, 0, (size_t)nwords * 8, A.stream));
        LAUNCH("merge", launch_merge_axpby(A.KA(1 - A.cur), A.vals[1 - A.cur], na, alpha, B.KA(1 - B.cur), B.vals[1 - B.cur], nb, beta,
                                           mk, mv, keep, A.stream));
        int64_t cnt = pack_small(A, KeyArr{mk, 1, 0}, mv, keep, 1, total, KeyArr{ok, 1, 0}, ov, total);
        if (cnt < 0) {
            LAUNCH("compact", launch_compact_range(KeyArr{mk, 1, 0}, mv, keep, 1, total, KeyArr{ok, 1, 0}, ov, total, &work, &cnt, A.stream));
        }
        if (cnt > cap) fail(DSA_ECAP, "output buffers too small");
        if (cnt > 0) {
            HIPCHK(hipMemcpyAsync(keys, ok, (size_t)cnt * 8, hipMemcpyDeviceToHost, A.stream));
            HIPCHK(hipMemcpyAsync(vals, ov, (size_t)cnt * 8, hipMemcpyDeviceToHost, A.stream));
            HIPCHK(hipStreamSynchronize(A.stream));
        }
        else HIPCHK(hipStreamSynchronize(A.stream));      // the scratch goes back to the pool: nothing may still use it
        *n_out = cnt;
    } catch (...) { (void)hipStreamSynchronize(A.stream); pool_free(scratch); throw; }
    pool_free(scratch);
    API_CATCH
}
int32_t dsa_vec_shrink_size(dsa_vec_t* h) {     // shrink_size!  src/vector.jl:64 (+ _guess_length :7-8)
    API_TRY
    vec_flush(h);
    std::vector<int64_t> ks; std::vector<double> vs;
    read_range(h->P, 1, h->P.capacity(), ks, vs);
    int64_t n = 0;
    for (int64_t k : ks) n = std::max(n, k);
    h->n = n;
    API_CATCH
}
int32_t dsa_vec_info(dsa_vec_t* h, int64_t* info) { API_TRY vec_flush(h); pma_info(h->P, h->n, info); API_CATCH }
int32_t dsa_vec_export_layout(dsa_vec_t* h, int64_t* keys, double* vals, uint8_t* occ, int64_t cap) {
    API_TRY vec_flush(h); export_slots(h->P, keys, vals, occ, cap); API_CATCH
}
int32_t dsa_vec_rebalance_root(dsa_vec_t* h) {
    API_TRY
    vec_flush(h);
    Pma& P = h->P;
    if (P.capacity() != P.h_ctl->segment_capacity) {
        P.h_ctl->stat_rebalances += 1; P.h_ctl->stat_window_slots += P.capacity();
        root_rebalance(P, P.capacity(), P.capacity(), P.h_ctl->nb_elements, false);
    }
    API_CATCH
}
int32_t dsa_vec_dev_relayout(dsa_vec_t* h, int32_t mode) {
    API_TRY
    vec_flush(h);
    Pma& P = h->P;
    Ctl& c = *P.h_ctl;
    const int64_t cap = c.capacity, m = c.nb_elements;
    if (m < 1) fail(DSA_EARG, "relayout of an empty vector");
    if (mode == 1 || mode == 2) {
        root_rebalance(P, cap, m, m, false);                   // W = m: no gaps -> the cells land on slots 1..m
        if (mode == 2) {
            const int alt = 1 - P.cur;
            ++P.layout_epoch;
            LAUNCH("pack-right", launch_pack_right(P.K(), P.V(), m, P.KA(alt), P.vals[alt], P.occ[alt], cap, P.stream));
            P.occ_dirty[alt] = std::max<int64_t>(P.occ_dirty[alt], (cap + 63) / 64);
            P.cur = alt;
        }
    } else if (mode == 3 || mode == 4) {
        if (mode == 4 && (cap < 4 * c.segment_capacity || 2 * m > cap)) fail(DSA_EARG, "cannot shrink");
        const int64_t old_cap = cap;
        if (mode == 3) { c.capacity *= 2; c.nb_segments *= 2; c.height += 1; } else { c.capacity /= 2; c.nb_segments /= 2; c.height -= 1; }
        compute_bounds(P);
        root_rebalance(P, old_cap, c.capacity, m, false);
        // (stream-ordered like the write path's own _extend! — which re-uploads the block with its relaunch —: no host wait in the hook)
        launch_check(launch_store_ctl(P.d_ctl, c, P.stream), "control block store: ");
    } else fail(DSA_EARG, "mode must be 1..4");
    API_CATCH
}
int32_t dsa_vec_check(dsa_vec_t* h, int64_t* report) { API_TRY vec_flush(h); pma_check(h->P, report); API_CATCH }
int32_t dsa_vec_set_stream(dsa_vec_t* h, void* s) {
    API_TRY
    vec_flush(h);
    HIPCHK(hipStreamSynchronize(h->P.stream));
    if (h->P.own_stream) stream_put(h->P.stream, h->P.device);
    h->P.stream = (hipStream_t)s; h->P.own_stream = false;
    API_CATCH
}
int32_t dsa_vec_sync(dsa_vec_t* h) { API_TRY vec_flush(h); HIPCHK(hipStreamSynchronize(h->P.stream)); API_CATCH }
int32_t dsa_vec_set_wait_policy(dsa_vec_t* h, int32_t policy) {
    API_TRY
    if (policy != DSA_WAIT_SPIN && policy != DSA_WAIT_BLOCK) fail(DSA_EARG, "wait policy must be DSA_WAIT_SPIN or DSA_WAIT_BLOCK");
    h->P.wait_policy = policy;
    API_CATCH
}

}  // extern "C"

extern "C" {

// ---------------- PackedCSC ----------------
int32_t dsa_pcsc_create(const int64_t* colptr, int64_t nparts, const int64_t* row_keys, const double* vals,
                        int32_t combine_op, dsa_pcsc_t** out) {
    API_TRY
    if (nparts <= 0) fail(DSA_EARG, "PackedCSC needs at least one partition");
    const int64_t nnz = colptr[nparts] - colptr[0];
    if (nnz > 0xffffffffll) fail(DSA_EARG, "more than 2^32-1 entries in one call");
    std::vector<int64_t> part((size_t)nnz);      // partition id of every entry (index expansion only; the sort / combine
    for (int64_t p = 0; p < nparts; ++p)          // of src/pcsr.jl:36-51 runs on the device)
        for (int64_t e = colptr[p]; e < colptr[p + 1]; ++e) part[(size_t)(e - colptr[0])] = p + 1;
    auto* h = new dsa_pcsc();
    try {
        pma_init_common(h->P, true, false);
        pma_build_from_host(h->P, part.data(), row_keys + colptr[0], vals + colptr[0], nnz, combine_op, 2, nparts);
    } catch (...) { pma_destroy(h->P); delete h; throw; }
    *out = h;
    API_CATCH
}
int32_t dsa_pcsc_create_empty(dsa_pcsc_t** out) {
    API_TRY
    auto* h = new dsa_pcsc();
    try {
        pma_init_common(h->P, true, false);
        ensure_tables(h->P, 64);
        build_from_packed(h->P, {}, {});
    } catch (...) { pma_destroy(h->P); delete h; throw; }
    *out = h;
    API_CATCH
}
int32_t dsa_pcsc_destroy(dsa_pcsc_t* h) { if (h) { pma_destroy(h->P); delete h; } return DSA_OK; }
int32_t dsa_pcsc_get(dsa_pcsc_t* h, int64_t key, int64_t partition, double* out) {
    API_TRY bind_device(h->P); get_batch(h->P, 1, &key, &partition, 1, out); API_CATCH
}
int32_t dsa_pcsc_set(dsa_pcsc_t* h, double val, int64_t key, int64_t partition) {
    API_TRY
    bind_device(h->P);
    if (partition > h->P.h_ctl->table_len + (1 << 24)) fail(DSA_EARG, "partition index unreasonably far past the last partition");
    std::vector<Op> ops{make_op(OP_PCSC_SET, key, partition, val)};
    int32_t err = 0;
    run_ops(h->P, ops, &err);
    if (err) fail(err, err_text(err));
    API_CATCH
}
int32_t dsa_pcsc_deletepartition(dsa_pcsc_t* h, int64_t partition) {
    API_TRY
    bind_device(h->P);
    std::vector<Op> ops{make_op(OP_DELETE_PARTITION, 0, partition, 0.0)};
    int32_t err = 0;
    run_ops(h->P, ops, &err);
    if (err) fail(err, err_text(err));
    API_CATCH
}
int32_t dsa_pcsc_nnz(dsa_pcsc_t* h, int64_t* out) { *out = h->P.h_ctl->nb_elements - h->P.h_ctl->nb_partitions; return DSA_OK; }
int32_t dsa_pcsc_nbpartitions(dsa_pcsc_t* h, int64_t* out) { *out = h->P.h_ctl->nb_partitions; return DSA_OK; }
int32_t dsa_pcsc_info(dsa_pcsc_t* h, int64_t* info) { pma_info(h->P, h->P.h_ctl->nb_partitions, info); return DSA_OK; }
int32_t dsa_pcsc_export_layout(dsa_pcsc_t* h, int64_t* keys, double* vals, uint8_t* occ, int64_t cap,
                               int64_t* semaphores, int64_t table_cap) {
    API_TRY
    bind_device(h->P);
    export_slots(h->P, keys, vals, occ, cap);
    export_tables(h->P, semaphores, nullptr, nullptr, table_cap);
    API_CATCH
}
int32_t dsa_pcsc_check(dsa_pcsc_t* h, int64_t* report) { API_TRY bind_device(h->P); pma_check(h->P, report); API_CATCH }

}  // extern "C"

extern "C" {

// ---------------- matrix ----------------
int32_t dsa_mat_create_from_coo(const int64_t* I, const int64_t* J, const double* V, int64_t nnz, int64_t m, int64_t n,
                                dsa_mat_t** out) {
    API_TRY
    if (nnz < 0) fail(DSA_EARG, "negative length");
    if (nnz > 0xffffffffll) fail(DSA_EARG, "more than 2^32-1 triples in one call");
    auto* h = new dsa_mat();
    KeyRange rows, cols;
    try { mat_build_major(h, I, J, V, nnz, &rows, &cols); mat_prefetch_spmv_meta(h); } catch (...) { mat_discard(h); throw; }
    if (m < 0) m = rows.known() ? std::max<int64_t>(0, rows.hi) : 0;        // _guess_length  src/vector.jl:6
    if (n < 0) n = cols.known() ? std::max<int64_t>(0, cols.hi) : 0;
    h->m = m; h->n = n;
    *out = h;
    API_CATCH
}
// dynamicsparse(I, J, V, m, n) with the triples in HBM, and the same from CSR / CSC arrays (ingest_host.hip)
int32_t dsa_mat_create_from_coo_dev(const void* d_I, const void* d_J, const double* d_V, int64_t nnz, int32_t index_bits, int32_t index_base,
                                    int64_t m, int64_t n, dsa_mat_t** out) {
    API_TRY
    *out = mat_from_coo_dev(d_I, d_J, d_V, nnz, index_bits, index_base, m, n);
    API_CATCH
}
int32_t dsa_mat_create_from_compressed_dev(int32_t orientation, int32_t index_bits, int32_t index_base, const void* d_ptr, const void* d_idx,
                                           const double* d_vals, int64_t outer, int64_t inner, int64_t nnz, dsa_mat_t** out) {
    API_TRY
    *out = mat_from_compressed_dev(orientation, index_bits, index_base, d_ptr, d_idx, d_vals, outer, inner, nnz);
    API_CATCH
}
// alpha * a + beta * shift(b) as a new matrix: copy, A + B, hcat, vcat, blockdiag (combine_host.hip)
int32_t dsa_mat_combine(dsa_mat_t* a, double alpha, dsa_mat_t* b, double beta, int64_t row_off, int64_t col_off, int64_t m, int64_t n,
                        dsa_mat_t** out) {
    API_TRY
    if (!a || !out) fail(DSA_EARG, "the first operand or out is NULL");
    *out = mat_combine(a, alpha, b, beta, row_off, col_off, m, n);
    API_CATCH
}
// ---------------- column-range shards (the reference is single-process) ----------------
// shard g of G owns the global column keys (col0, col0 + ncols]: n / G columns each, the first n % G shards one more
int32_t dsa_shard_range(int64_t n, int32_t nshards, int32_t shard, int64_t* col0, int64_t* ncols) {
    API_TRY
    if (n < 0 || nshards <= 0 || shard < 0 || shard >= nshards) fail(DSA_EARG, "shard index / count out of range");
    const int64_t base = n / nshards, rem = n % nshards;
    *col0 = shard * base + std::min<int64_t>(shard, rem);
    *ncols = base + (shard < rem ? 1 : 0);
    API_CATCH
}
// the shard's sub-matrix as an independent reference-layout matrix: the triples whose column lies in the shard's range, with
// LOCAL column keys 1..ncols (so x is the shard's slice of the global x); size m x ncols
int32_t dsa_shard_create_from_coo(const int64_t* I, const int64_t* J, const double* V, int64_t nnz, int64_t m, int64_t n,
                                  int32_t nshards, int32_t shard, dsa_mat_t** out) {
    int64_t col0 = 0, ncols = 0;
    if (n < 0) { g_err = "a sharded matrix needs its global column count"; return DSA_EARG; }
    const int32_t rc = dsa_shard_range(n, nshards, shard, &col0, &ncols);
    if (rc != DSA_OK) return rc;
    std::vector<int64_t> li, lj; std::vector<double> lv;
    try {
        for (int64_t k = 0; k < nnz; ++k)
            if (J[k] > col0 && J[k] <= col0 + ncols) { li.push_back(I[k]); lj.push_back(J[k] - col0); lv.push_back(V[k]); }
    } catch (const std::bad_alloc&) { g_err = "host allocation failed"; return DSA_EHIP; }
    return dsa_mat_create_from_coo(li.data(), lj.data(), lv.data(), (int64_t)li.size(), m, ncols, out);
}
// partial y (length m) of one shard: y_g = A[:, range_g] * x[range_g], x and y resident in HBM, asynchronous on the handle's
// stream; the all-reduce over the shards belongs to the host layer (RCCL through torch.distributed, one process per GPU)
int32_t dsa_shard_spmv_dev(dsa_mat_t* h, const double* d_x_local, int64_t nx, double* d_y_partial, int64_t ny) {
    return dsa_mat_spmv_dense_dev(h, 0, 0, d_x_local, nx, d_y_partial, ny);
}
// y = A x of the whole sharded matrix: the local product, then the RCCL all-reduce of the partial y over the ranks (comm.hip),
// both on the shard's stream — the one collective of the path, entirely behind the ABI (dsa_shard_spmv)
int32_t dsa_shard_spmv_allreduce_dev(dsa_mat_t* h, dsa_comm_t* comm, const double* d_x_local, int64_t nx, double* d_y, int64_t ny) {
    const int32_t rc = dsa_mat_spmv_dense_dev(h, 0, 0, d_x_local, nx, d_y, ny);
    if (rc != DSA_OK) return rc;
    return dsa_shard_allreduce_dev(comm, d_y, ny, h->row.stream);
}
int32_t dsa_mat_create_empty(int32_t fill_mode, dsa_mat_t** out) {
    API_TRY
    auto* h = new dsa_mat();
    if (fill_mode) {
        HIPCHK(hipSetDevice(g_device));     // fail loudly without a device even though nothing is allocated yet
        h->fillmode = true;
    } else {
        try { mat_build_major(h, nullptr, nullptr, nullptr, 0); } catch (...) { mat_discard(h); throw; }
    }
    *out = h;
    API_CATCH
}
int32_t dsa_mat_destroy(dsa_mat_t* h) {
    if (h) {
        if (h->has_major) { pma_destroy(h->col); pma_destroy(h->row); }
        fill_release(h->buf);
        if (h->d_x) hipFree(h->d_x);
        if (h->d_y) hipFree(h->d_y);
        {
            dsa_mat::Spx& x = h->spx;
            if (x.res_stream) (void)hipStreamSynchronize(x.res_stream);
            pool_free(x.acc); pool_free(x.bm); pool_free(x.tile_cnt); pool_free(x.tile_off); pool_free(x.ticket);
            pool_free(x.oi); pool_free(x.ov); pool_free(x.dx); pool_free(x.d_count);
            pinned_free(x.pin);
            for (hipEvent_t e : x.ev) if (e) (void)hipEventDestroy(e);
            if (x.stage) (void)hipHostFree(x.stage);
        }
        delete h;
    }
    return DSA_OK;
}

int32_t dsa_mat_set(dsa_mat_t* h, double val, int64_t row, int64_t col) {
    API_TRY
    check_key(row); check_key(col);
    if (val != 0.0) { h->m = std::max(h->m, row); h->n = std::max(h->n, col); }      // src/matrix.jl:44-47
    if (h->fillmode) {
        fill_row_test_and_set(h->buf, row);
        fill_append(h->buf, &row, &col, &val, 1);
    } else {
        mat_content_changed(h);
        h->pi.push_back(row); h->pj.push_back(col); h->pv.push_back(val);
        // with tombstones a write can hit the reference's assert / bounds paths: apply it now so the error surfaces here
        const bool tombstones = h->col.h_ctl->nb_partitions != h->col.h_ctl->table_len ||
                                h->row.h_ctl->nb_partitions != h->row.h_ctl->table_len;
        if (tombstones || h->pi.size() >= PENDING_FLUSH) mat_flush(h);
    }
    API_CATCH
}

int32_t dsa_mat_set_batch(dsa_mat_t* h, const int64_t* I, const int64_t* J, const double* V, int64_t n) {
    API_TRY
    for (int64_t k = 0; k < n; ++k) { check_key(I[k]); check_key(J[k]); }
    mat_flush(h);
    if (h->fillmode) {
        for (int64_t k = 0; k < n; ++k) {
            if (V[k] != 0.0) { h->m = std::max(h->m, I[k]); h->n = std::max(h->n, J[k]); }
            fill_row_test_and_set(h->buf, I[k]);
        }
        fill_append(h->buf, I, J, V, n);
    } else {
        mat_content_changed(h);
        mat_apply_sets(h, I, J, V, n);
        mat_prefetch_spmv_meta(h);
    }
    API_CATCH
}

int32_t dsa_mat_get_batch(dsa_mat_t* h, const int64_t* I, const int64_t* J, int64_t n, double* out) {
    API_TRY
    mat_flush(h);
    if (h->fillmode) fail(DSA_EMODE, "getindex(row, col) is not available in fill mode.");
    get_batch(h->col, 2, I, J, n, out);
    API_CATCH
}
int32_t dsa_mat_get(dsa_mat_t* h, int64_t row, int64_t col, double* out) { return dsa_mat_get_batch(h, &row, &col, 1, out); }

int32_t dsa_mat_addrow(dsa_mat_t* h, int64_t row, const int64_t* colids, const double* vals, int64_t n) {
    API_TRY
    mat_flush(h);
    check_key(row);
    for (int64_t k = 0; k < n; ++k) check_key(colids[k]);
    if (h->fillmode) {     // addrow!(buffer, ...)  src/buffer.jl:10-18
        FillBuffer& b = h->buf;
        if (fill_row_test_and_set(b, row)) fail(DSA_EMODE, "Row already written in dynamic sparse matrix buffer.");
        std::vector<int64_t> rows((size_t)n, row);       // (the reference stores the column ids of the row sorted: only its buffer views see that)
        fill_append(b, rows.data(), colids, vals, n);
    } else {               // src/matrix.jl:119-121
        mat_content_changed(h);
        std::vector<int64_t> rows((size_t)n, row);
        mat_apply_sets(h, rows.data(), colids, vals, n);
        mat_prefetch_spmv_meta(h);
    }
    API_CATCH
}

int32_t dsa_mat_closefillmode(dsa_mat_t* h) {     // closefillmode!  src/matrix.jl:126-134
    API_TRY
    mat_flush(h);
    if (!h->fillmode) fail(DSA_EMODE, "Cannot close fill mode because matrix is not in fill mode.");
    mat_content_changed(h);
    const auto tc0 = Clock::now();
    const FillDrain d = fill_drain(h->buf);
    // (the nnz > 0 guard stays here: needs_wide says wide for an UNKNOWN range under DSA_KEYS_WIDE=1, an empty buffer always closed narrow)
    const bool wr = d.nnz > 0 && needs_wide(d.rows), wc = d.nnz > 0 && needs_wide(d.cols);
    // a failed build (out of memory, a HIP error) leaves the matrix what it was: in fill mode, with all of its triples — the
    // builder only reads them — so the caller may free memory and close again, or keep appending
    const auto tc1 = Clock::now();
    mat_build_major_dev(h, h->buf.dI, h->buf.dJ, h->buf.dV, d.nnz, wr, wc, d.rows, d.cols);
    const auto tc2 = Clock::now();
    h->fillmode = false;
    fill_release(h->buf);
    mat_prefetch_spmv_meta(h);
    if (dbg_time())
        fprintf(stderr, "[closefillmode] last chunk %.2f ms  build %.2f ms  release + prefetch %.2f ms\n", elapsed_ms(tc0, tc1), elapsed_ms(tc1, tc2), elapsed_ms(tc2));
    API_CATCH
}

int32_t dsa_mat_deletecolumn(dsa_mat_t* h, int64_t col) {      // src/matrix.jl:95-102
    API_TRY
    mat_flush(h);
    if (h->fillmode) fail(DSA_EMODE, "Cannot delete a column in fill mode");
    mat_content_changed(h);
    mat_delete_partition(h, DSA_COLMAJOR, col);
    API_CATCH
}
int32_t dsa_mat_deleterow(dsa_mat_t* h, int64_t row) {         // src/matrix.jl:104-111
    API_TRY
    mat_flush(h);
    if (h->fillmode) fail(DSA_EMODE, "Cannot delete a row in fill mode");
    mat_content_changed(h);
    mat_delete_partition(h, DSA_ROWMAJOR, row);
    API_CATCH
}

int32_t dsa_mat_col_view(dsa_mat_t* h, int64_t col, int64_t* rows, double* vals, int64_t cap, int64_t* n_out) {
    return view_impl(h, DSA_COLMAJOR, col, rows, vals, cap, n_out);
}
int32_t dsa_mat_row_view(dsa_mat_t* h, int64_t row, int64_t* cols, double* vals, int64_t cap, int64_t* n_out) {
    return view_impl(h, DSA_ROWMAJOR, row, cols, vals, cap, n_out);
}
int32_t dsa_mat_col_view_dev(dsa_mat_t* h, int64_t col, int64_t* d_rows, double* d_vals, int64_t cap, int64_t* n_out) {
    return view_dev_impl(h, DSA_COLMAJOR, col, d_rows, d_vals, cap, n_out);
}
int32_t dsa_mat_row_view_dev(dsa_mat_t* h, int64_t row, int64_t* d_cols, double* d_vals, int64_t cap, int64_t* n_out) {
    return view_dev_impl(h, DSA_ROWMAJOR, row, d_cols, d_vals, cap, n_out);
}
int32_t dsa_mat_col_slice(dsa_mat_t* h, int64_t col, dsa_vec_t** out) { return slice_impl(h, DSA_COLMAJOR, col, out); }
int32_t dsa_mat_row_slice(dsa_mat_t* h, int64_t row, dsa_vec_t** out) { return slice_impl(h, DSA_ROWMAJOR, row, out); }

int32_t dsa_mat_nnz(dsa_mat_t* h, int64_t* out) {      // nnz(m) = nnz(m.rowmajor)  src/matrix.jl:91
    API_TRY mat_flush(h); Pma& P = orient(h, DSA_ROWMAJOR); *out = P.h_ctl->nb_elements - P.h_ctl->nb_partitions; API_CATCH
}
int32_t dsa_mat_size(dsa_mat_t* h, int64_t* m, int64_t* n) { *m = h->m; *n = h->n; return DSA_OK; }
int32_t dsa_mat_nbpartitions(dsa_mat_t* h, int32_t o, int64_t* out) { API_TRY mat_flush(h); *out = orient(h, o).h_ctl->nb_partitions; API_CATCH }
int32_t dsa_mat_info(dsa_mat_t* h, int32_t o, int64_t* info) { API_TRY mat_flush(h); Pma& P = orient(h, o); pma_info(P, P.h_ctl->nb_partitions, info); API_CATCH }
int32_t dsa_mat_export_layout(dsa_mat_t* h, int32_t o, int64_t* keys, double* vals, uint8_t* occ, int64_t cap,
                              int64_t* semaphores, int64_t* col_keys, uint8_t* col_live, int64_t table_cap) {
    API_TRY
    mat_flush(h);
    Pma& P = orient(h, o);
    export_slots(P, keys, vals, occ, cap);
    export_tables(P, semaphores, col_keys, col_live, table_cap);
    API_CATCH
}
int32_t dsa_mat_rebalance_root(dsa_mat_t* h, int32_t o) {
    API_TRY
    mat_flush(h);
    mat_content_changed(h);
    Pma& P = orient(h, o);
    if (P.capacity() != P.h_ctl->segment_capacity) {
        P.h_ctl->stat_rebalances += 1; P.h_ctl->stat_window_slots += P.capacity();
        root_rebalance(P, P.capacity(), P.capacity(), P.h_ctl->nb_elements, false);
    }
    API_CATCH
}

int32_t dsa_mat_to_compressed_dev(dsa_mat_t* h, int32_t orientation, int32_t index_bits, int32_t index_base,
                                  void* d_ptr, void* d_idx, double* d_vals, int64_t cap, int64_t* nnz_out) {
    API_TRY
    to_compressed_dev(h, orientation, index_bits, index_base, d_ptr, d_idx, d_vals, cap, nnz_out);
    API_CATCH
}
int32_t dsa_mat_to_compressed(dsa_mat_t* h, int32_t orientation, int32_t index_base,
                              int64_t* ptr, int64_t* idx, double* vals, int64_t cap, int64_t* nnz_out) {
    API_TRY
    to_compressed_host(h, orientation, index_base, ptr, idx, vals, cap, nnz_out);
    API_CATCH
}

// ---- selected export (select.hip): the partitions of a key list as one CSC / CSR; read-only like the full export
int32_t dsa_mat_select_compressed_dev(dsa_mat_t* h, int32_t orientation, int32_t index_bits, int32_t index_base,
                                      const int64_t* d_sel, int64_t nsel,
                                      void* d_ptr, void* d_idx, double* d_vals, int64_t cap, int64_t* nnz_out) {
    API_TRY
    select_compressed_dev(h, orientation, index_bits, index_base, d_sel, nsel, d_ptr, d_idx, d_vals, cap, nnz_out);
    API_CATCH
}
int32_t dsa_mat_select_compressed(dsa_mat_t* h, int32_t orientation, int32_t index_base,
                                  const int64_t* sel, int64_t nsel,
                                  int64_t* ptr, int64_t* idx, double* vals, int64_t cap, int64_t* nnz_out) {
    API_TRY
    select_compressed_host(h, orientation, index_base, sel, nsel, ptr, idx, vals, cap, nnz_out);
    API_CATCH
}

// ---- submatrix export (submatrix.hip): A[I, J] with both key lists as one CSC / CSR; read-only like the selected export
int32_t dsa_mat_submatrix_compressed_dev(dsa_mat_t* h, int32_t orientation, int32_t index_bits, int32_t index_base,
                                         const int64_t* d_outer, int64_t nouter, const int64_t* d_inner, int64_t ninner,
                                         void* d_ptr, void* d_idx, double* d_vals, int64_t cap, int64_t* nnz_out) {
    API_TRY
    submatrix_compressed_dev(h, orientation, index_bits, index_base, d_outer, nouter, d_inner, ninner, d_ptr, d_idx, d_vals, cap, nnz_out);
    API_CATCH
}
int32_t dsa_mat_submatrix_compressed(dsa_mat_t* h, int32_t orientation, int32_t index_base,
                                     const int64_t* outer, int64_t nouter, const int64_t* inner, int64_t ninner,
                                     int64_t* ptr, int64_t* idx, double* vals, int64_t cap, int64_t* nnz_out) {
    API_TRY
    submatrix_compressed_host(h, orientation, index_base, outer, nouter, inner, ninner, ptr, idx, vals, cap, nnz_out);
    API_CATCH
}

int32_t dsa_mat_spmv_dense_dev(dsa_mat_t* h, int32_t transpose, int32_t algo, const double* d_x, int64_t nx, double* d_y, int64_t ny) {
    API_TRY
    mat_flush(h);
    Pma& P = transpose ? h->col : h->row;
    spmv_dev(h, transpose, algo, d_x, nx, d_y, ny, P.stream);
    API_CATCH
}

int32_t dsa_mat_spmv_dense(dsa_mat_t* h, int32_t transpose, const double* x, int64_t nx, double* y, int64_t ny) {
    API_TRY
    mat_flush(h);
    if (!h->has_major) fail(DSA_EMODE, "matrix is in fill mode");
    if (nx < 0 || ny < 0) fail(DSA_EARG, "negative length");
    ensure_xy(h, nx, ny);
    Pma& P = transpose ? h->col : h->row;
    if (nx > 0) HIPCHK(hipMemcpyAsync(h->d_x, x, (size_t)nx * sizeof(double), hipMemcpyHostToDevice, P.stream));
    if (ny > 0) {
        spmv_dev(h, transpose, 0, h->d_x, nx, h->d_y, ny, P.stream);
        HIPCHK(hipMemcpyAsync(y, h->d_y, (size_t)ny * sizeof(double), hipMemcpyDeviceToHost, P.stream));
    }
    HIPCHK(hipStreamSynchronize(P.stream));
    API_CATCH
}

int32_t dsa_mat_spmm_dense_dev(dsa_mat_t* h, int32_t transpose, const double* d_x, int64_t nx, int64_t k, int64_t ldx,
                               double* d_y, int64_t ny, int64_t ldy) {
    API_TRY
    mat_flush(h);
    Pma& P = transpose ? h->col : h->row;
    spmm_dev(h, transpose, d_x, nx, k, ldx, d_y, ny, ldy, P.stream);
    API_CATCH
}

int32_t dsa_mat_spmm_dense(dsa_mat_t* h, int32_t transpose, const double* x, int64_t nx, int64_t k, int64_t ldx,
                           double* y, int64_t ny, int64_t ldy) {
    API_TRY
    spmm_host(h, transpose, x, nx, k, ldx, y, ny, ldy);
    API_CATCH
}

int32_t dsa_mat_spmm_selected_dev(dsa_mat_t* h, int32_t transpose, const int64_t* d_sel, int64_t nsel, const double* d_x, int64_t nx,
                                  int64_t k, int64_t ldx, double* d_y, int64_t ldy) {
    API_TRY
    mat_flush(h);
    Pma& P = transpose ? h->col : h->row;
    selprod_dev(h, transpose, d_sel, nsel, d_x, nx, k, ldx, d_y, ldy, P.stream);
    API_CATCH
}

int32_t dsa_mat_spmm_selected(dsa_mat_t* h, int32_t transpose, const int64_t* sel, int64_t nsel, const double* x, int64_t nx,
                              int64_t k, int64_t ldx, double* y, int64_t ldy) {
    API_TRY
    selprod_host(h, transpose, sel, nsel, x, nx, k, ldx, y, ldy);
    API_CATCH
}

// ---- batched sparse-x product (spgemm.hip): Y = A S / A' S, operands and result CSC; read-only like the exports
int32_t dsa_mat_spgemm_csc_dev(dsa_mat_t* h, int32_t transpose, int32_t index_bits, int32_t index_base,
                               const void* d_xptr, const void* d_xidx, const double* d_xval, int64_t k, int64_t nnzx,
                               void* d_yptr, void* d_yidx, double* d_yval, int64_t cap, int64_t* nnz_out) {
    API_TRY
    spgemm_csc_dev(h, transpose, index_bits, index_base, d_xptr, d_xidx, d_xval, k, nnzx, d_yptr, d_yidx, d_yval, cap, nnz_out);
    API_CATCH
}
int32_t dsa_mat_spgemm_csc(dsa_mat_t* h, int32_t transpose, int32_t index_base,
                           const int64_t* xptr, const int64_t* xidx, const double* xval, int64_t k,
                           int64_t* yptr, int64_t* yidx, double* yval, int64_t cap, int64_t* nnz_out) {
    API_TRY
    spgemm_csc_host(h, transpose, index_base, xptr, xidx, xval, k, yptr, yidx, yval, cap, nnz_out);
    API_CATCH
}

// ---- reductions per row / column (scale.hip): read-only
int32_t dsa_mat_reduce_dev(dsa_mat_t* h, int32_t orientation, int32_t kind, double* d_out, int64_t n_out) {
    API_TRY
    reduce_dev(h, orientation, kind, d_out, n_out);
    API_CATCH
}
int32_t dsa_mat_reduce(dsa_mat_t* h, int32_t orientation, int32_t kind, double* out, int64_t n_out) {
    API_TRY
    reduce_host(h, orientation, kind, out, n_out);
    API_CATCH
}

// ---- the batched read that stays in HBM (update_host.hip)
int32_t dsa_mat_get_batch_dev(dsa_mat_t* h, const int64_t* d_I, const int64_t* d_J, int64_t n, double* d_out, uint8_t* d_found) {
    API_TRY
    get_batch_dev(h, d_I, d_J, n, d_out, d_found);
    API_CATCH
}

int32_t dsa_mat_check(dsa_mat_t* h, int32_t o, int64_t* report) { API_TRY mat_flush(h); pma_check(orient(h, o), report); API_CATCH }
int32_t dsa_mat_set_stream(dsa_mat_t* h, void* s) {
    API_TRY
    mat_flush(h);
    if (!h->has_major) fail(DSA_EMODE, "matrix is in fill mode");
    for (Pma* P : {&h->col, &h->row}) {
        HIPCHK(hipStreamSynchronize(P->stream));
        if (P->own_stream) stream_put(P->stream, P->device);
        P->stream = (hipStream_t)s; P->own_stream = false;
    }
    API_CATCH
}
int32_t dsa_mat_set_wait_policy(dsa_mat_t* h, int32_t policy) {
    API_TRY
    if (policy != DSA_WAIT_SPIN && policy != DSA_WAIT_BLOCK) fail(DSA_EARG, "wait policy must be DSA_WAIT_SPIN or DSA_WAIT_BLOCK");
    h->col.wait_policy = policy; h->row.wait_policy = policy;
    API_CATCH
}
int32_t dsa_mat_sync(dsa_mat_t* h) {
    API_TRY
    mat_flush(h);
    if (h->has_major) { HIPCHK(hipStreamSynchronize(h->col.stream)); HIPCHK(hipStreamSynchronize(h->row.stream)); }
    API_CATCH
}

}  // extern "C"
