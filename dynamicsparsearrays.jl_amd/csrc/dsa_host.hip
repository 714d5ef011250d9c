// csrc/dsa_host.hip — the handle layer of libdsa_hip.so: the last-error text, the table of development switches, the fill-mode
// staging buffer, what is written in terms of dsa_vec / dsa_pcsc / dsa_mat (flush and apply of queued writes, the builds of both
// orientations, slices, the dense product) and the C ABI of include/dsa.h.
//
// Everything that works on ONE packed-memory array (the Pma of host.h) is in the engine units pma_host.hip (lifecycle, geometry,
// rebalances, reads), writes_host.hip (yield loop around the sequencer, batch-parallel rounds), build_host.hip (K-build) and
// spmv_host.hip (SpMV meta and plan); the exports, the multi-vector product and the device import sit behind three-line entry points
// in export_host.hip, spmm_host.hip, selprod_host.hip and ingest_host.hip; the sparse-x product and the parity hooks have entry points of their own in
// sparsex_host.hip and raw_host.hip.
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
#include <exception>
#include <mutex>
#include <string>
#include <thread>
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
inline bool fill_row_test_and_set(FillBuffer& b, int64_t row) {
    if (row >= 1 && row < ((int64_t)1 << 28)) {
        const size_t w = (size_t)(row >> 6);
        if (w >= b.row_bits.size()) b.row_bits.resize(std::max<size_t>(2 * b.row_bits.size(), w + 1024), 0ull);
        const uint64_t bit = 1ull << (row & 63);
        const bool was = (b.row_bits[w] & bit) != 0;
        b.row_bits[w] |= bit;
        return was;
    }
    return !b.rows_far.insert(row).second;
}
// pinned staging chunks are expensive to allocate and free (milliseconds each): one set is kept for the next fill-mode matrix
struct FillStagingCache { std::mutex mu; int64_t* hI[2] = {nullptr, nullptr}; int64_t* hJ[2] = {nullptr, nullptr}; double* hV[2] = {nullptr, nullptr}; int device = -1; };
static FillStagingCache g_fill_cache;
void fill_release(FillBuffer& b) {
    if (b.stream) hipStreamSynchronize(b.stream);
    {
        std::lock_guard<std::mutex> lk(g_fill_cache.mu);
        if (b.hI[0] && g_fill_cache.hI[0] == nullptr) {
            for (int k = 0; k < 2; ++k) { g_fill_cache.hI[k] = b.hI[k]; g_fill_cache.hJ[k] = b.hJ[k]; g_fill_cache.hV[k] = b.hV[k]; b.hI[k] = nullptr; b.hJ[k] = nullptr; b.hV[k] = nullptr; }
            g_fill_cache.device = b.device;
        }
    }
    for (int k = 0; k < 2; ++k) {
        if (b.hI[k]) hipHostFree(b.hI[k]);
        if (b.hJ[k]) hipHostFree(b.hJ[k]);
        if (b.hV[k]) hipHostFree(b.hV[k]);
        if (b.uploaded[k]) hipEventDestroy(b.uploaded[k]);
    }
    pool_free(b.dI); pool_free(b.dJ); pool_free(b.dV);
    pool_free(b.d_acc); pinned_free(b.h_acc);
    if (b.stream) stream_put(b.stream, b.device);
    b = FillBuffer();
}

// ---- device-resident fill buffer --------------------------------------------------------------------------------------
void fill_init(FillBuffer& b) {
    if (b.stream) return;
    HIPCHK(hipSetDevice(g_device));
    b.device = g_device;
    HIPCHK(stream_get(&b.stream));
    {
        std::lock_guard<std::mutex> lk(g_fill_cache.mu);
        if (g_fill_cache.hI[0] != nullptr && g_fill_cache.device == b.device)
            for (int k = 0; k < 2; ++k) { b.hI[k] = g_fill_cache.hI[k]; b.hJ[k] = g_fill_cache.hJ[k]; b.hV[k] = g_fill_cache.hV[k]; g_fill_cache.hI[k] = nullptr; g_fill_cache.hJ[k] = nullptr; g_fill_cache.hV[k] = nullptr; }
    }
    {
        void* p = nullptr;
        HIPCHK(pool_alloc(&p, 64)); b.d_acc = static_cast<long long*>(p);
        HIPCHK(pinned_alloc(&p, 64)); b.h_acc = static_cast<long long*>(p);
        b.h_acc[0] = INT64_MAX; b.h_acc[1] = INT64_MIN; b.h_acc[2] = INT64_MAX; b.h_acc[3] = INT64_MIN; b.h_acc[4] = 0;
        HIPCHK(hipMemcpyAsync(b.d_acc, b.h_acc, 5 * sizeof(long long), hipMemcpyHostToDevice, b.stream));
        HIPCHK(hipStreamSynchronize(b.stream));             // (h_acc is reused as the read-back target)
    }
    for (int k = 0; k < 2; ++k) {
        HIPCHK(hipEventCreateWithFlags(&b.uploaded[k], hipEventDisableTiming));
        if (b.hI[k]) continue;
        HIPCHK(hipHostMalloc(&b.hI[k], (size_t)FillBuffer::CHUNK * sizeof(int64_t), hipHostMallocDefault));
        HIPCHK(hipHostMalloc(&b.hJ[k], (size_t)FillBuffer::CHUNK * sizeof(int64_t), hipHostMallocDefault));
        HIPCHK(hipHostMalloc(&b.hV[k], (size_t)FillBuffer::CHUNK * sizeof(double), hipHostMallocDefault));
    }
}
// ships what is staged in the current pinned chunk and not yet sent (triples [b.sent, b.fill)) to HBM, asynchronously; a chunk that
// is full (or `finish`: the end of a batch) is closed — its event recorded — and the other chunk becomes current.  Pieces go up
// while the caller's memcpy fills the rest of the chunk, so that closefillmode! waits for one piece (6 MB), not for a chunk (24 MB).
void fill_upload_chunk(FillBuffer& b, bool finish = true) {
    if (b.fill == 0) return;
    HIPCHK(hipSetDevice(b.device));
    const int64_t npiece = b.fill - b.sent;
    if (npiece > 0) {
        if (b.dlen + npiece > b.dcap) {          // grow geometrically: new arrays, device-to-device copy of what is resident
            const int64_t ncap = std::max<int64_t>(2 * b.dcap, std::max<int64_t>(b.dlen + npiece, 4 * FillBuffer::CHUNK));
            int64_t *nI = nullptr, *nJ = nullptr; double* nV = nullptr;
            HIPCHK(pool_alloc(reinterpret_cast<void**>(&nI), (size_t)ncap * sizeof(int64_t)));
            HIPCHK(pool_alloc(reinterpret_cast<void**>(&nJ), (size_t)ncap * sizeof(int64_t)));
            HIPCHK(pool_alloc(reinterpret_cast<void**>(&nV), (size_t)ncap * sizeof(double)));
            if (b.dlen > 0) {
                HIPCHK(hipMemcpyAsync(nI, b.dI, (size_t)b.dlen * sizeof(int64_t), hipMemcpyDeviceToDevice, b.stream));
                HIPCHK(hipMemcpyAsync(nJ, b.dJ, (size_t)b.dlen * sizeof(int64_t), hipMemcpyDeviceToDevice, b.stream));
                HIPCHK(hipMemcpyAsync(nV, b.dV, (size_t)b.dlen * sizeof(double), hipMemcpyDeviceToDevice, b.stream));
            }
            HIPCHK(hipStreamSynchronize(b.stream));       // earlier uploads into the old arrays have landed
            pool_free(b.dI); pool_free(b.dJ); pool_free(b.dV);
            b.dI = nI; b.dJ = nJ; b.dV = nV; b.dcap = ncap;
        }
        const int c = b.cur;
        HIPCHK(hipMemcpyAsync(b.dI + b.dlen, b.hI[c] + b.sent, (size_t)npiece * sizeof(int64_t), hipMemcpyHostToDevice, b.stream));
        HIPCHK(hipMemcpyAsync(b.dJ + b.dlen, b.hJ[c] + b.sent, (size_t)npiece * sizeof(int64_t), hipMemcpyHostToDevice, b.stream));
        HIPCHK(hipMemcpyAsync(b.dV + b.dlen, b.hV[c] + b.sent, (size_t)npiece * sizeof(double), hipMemcpyHostToDevice, b.stream));
        {   // the value ranges of the piece, folded into the running ones behind its upload
            LAUNCH("key range", launch_key_scan_acc(b.dI + b.dlen, b.dJ + b.dlen, npiece, b.d_acc, b.stream));
        }
        b.dlen += npiece;
        b.sent = b.fill;
    }
    if (!finish && b.fill < FillBuffer::CHUNK) return;
    const int c = b.cur;
    HIPCHK(hipEventRecord(b.uploaded[c], b.stream));
    b.in_flight[c] = true;
    b.fill = 0; b.sent = 0;
    b.cur = 1 - c;
    if (b.in_flight[b.cur]) { HIPCHK(hipEventSynchronize(b.uploaded[b.cur])); b.in_flight[b.cur] = false; }   // its pinned memory is free again
}
// addelem!  src/buffer.jl:20-31 for n entries (n = 1: one setindex! in fill mode)
void fill_append(FillBuffer& b, const int64_t* I, const int64_t* J, const double* V, int64_t n) {
    fill_init(b);
    int64_t k = 0;
    while (k < n) {
        const int64_t room = std::min(FillBuffer::CHUNK - b.fill, FillBuffer::PIECE - (b.fill - b.sent));      // up to the end of the chunk / of the piece
        const int64_t take = std::min(room, n - k);
        std::memcpy(b.hI[b.cur] + b.fill, I + k, (size_t)take * sizeof(int64_t));
        std::memcpy(b.hJ[b.cur] + b.fill, J + k, (size_t)take * sizeof(int64_t));
        std::memcpy(b.hV[b.cur] + b.fill, V + k, (size_t)take * sizeof(double));
        b.fill += take; k += take;
        if (b.fill == FillBuffer::CHUNK || b.fill - b.sent >= FillBuffer::PIECE) fill_upload_chunk(b, false);
    }
    // a batch of appends has ended: what is staged goes up now (asynchronously), so that closefillmode! finds almost nothing left
    // in pinned memory — single-element appends (setindex! in fill mode) only ship whole quarter chunks
    if (b.fill - b.sent >= (n > 1 ? FillBuffer::EAGER : FillBuffer::CHUNK / 4)) fill_upload_chunk(b, false);
    b.length += n;
}

void bind_device(const Pma& P) { HIPCHK(hipSetDevice(P.device)); }
void check_key(int64_t k) { if (k == 0) fail(DSA_EKEY, "0 is the reserved semaphore key (src/pcsr.jl:23)"); }
Op make_op(int32_t kind, int64_t a, int64_t b, double v) { Op o; o.a = a; o.b = b; o.v = v; o.kind = kind; o.pad = 0; return o; }
Pma& orient(dsa_mat* h, int32_t o) {
    if (!h->has_major) fail(DSA_EMODE, "matrix is in fill mode");
    if (o != DSA_COLMAJOR && o != DSA_ROWMAJOR) fail(DSA_EARG, "orientation must be 0 or 1");
    return o == DSA_COLMAJOR ? h->col : h->row;
}

// both orientations from (row, col, value) triples that are ALREADY in HBM (they stay the caller's): dynamicsparse(I, J, V) after its
// upload, closefillmode! straight from the device-resident fill buffer.  On failure nothing of the two structures is left behind.
void mat_build_major_dev(dsa_mat* h, const int64_t* dI, const int64_t* dJ, const double* dV, int64_t nnz, bool wide_rows, bool wide_cols,
                         KeyRange rows = KeyRange(), KeyRange cols = KeyRange()) {
    try {
        static const bool dbg_time = dev_env("DSA_DBG_TIME") != nullptr;
        const auto ti0 = std::chrono::steady_clock::now();
        pma_init_common(h->col, true, true);
        pma_init_common(h->row, true, true);
        const auto tb0 = std::chrono::steady_clock::now();
        if (dbg_time) fprintf(stderr, "[mat_build_major] handles (streams, control blocks) %.2f ms\n", std::chrono::duration<double, std::milli>(tb0 - ti0).count());
        // the two orientations are independent structures on their own streams and both only read the triples: built side by side
        // (the rowmajor one on a helper thread; each build waits once for its cell / partition counts)
        // large builds: ONE sort of the triples, the rowmajor orientation from the cells colmajor's emit leaves behind (mat_build_both_dev);
        // smaller ones, a shared stream or an injected failure: two independent builds side by side
        if (nnz >= (1 << 16) && h->col.stream != h->row.stream && dev_env("DSA_FAIL_BUILD") == nullptr) {
            const bool both = mat_build_both_dev(h->col, h->row, dJ, dI, dV, nnz, wide_rows, wide_cols, cols, rows);
            if (!both) pma_build_dev(h->row, dI, dJ, dV, nnz, DSA_COMBINE_ADD, 0, 0, wide_cols, rows, cols);
            if (dbg_time) fprintf(stderr, "[mat_build_major] nnz=%lld both orientations (%s) %.1f ms\n", (long long)nnz, both ? "twin derived" : "general path",
                                  std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tb0).count());
            h->has_major = true;
            return;
        }
        std::exception_ptr row_exc;
        std::thread row_thread;
        const bool side_by_side = h->col.stream != h->row.stream && nnz > 0;
        if (side_by_side)
            row_thread = std::thread([&] {
                try { bind_device(h->row); pma_build_dev(h->row, dI, dJ, dV, nnz, DSA_COMBINE_ADD, 0, 0, wide_cols, rows, cols); }
                catch (...) { row_exc = std::current_exception(); }
            });
        try { pma_build_dev(h->col, dJ, dI, dV, nnz, DSA_COMBINE_ADD, 0, 0, wide_rows, cols, rows); }      // dynamicsparsecolmajor(I, J, V): partitions = columns, keys = rows
        catch (...) { if (row_thread.joinable()) row_thread.join(); throw; }
        const auto tb1 = std::chrono::steady_clock::now();
        if (side_by_side) { row_thread.join(); if (row_exc) std::rethrow_exception(row_exc); }
        else pma_build_dev(h->row, dI, dJ, dV, nnz, DSA_COMBINE_ADD, 0, 0, wide_cols, rows, cols);      // dynamicsparsecolmajor(J, I, V): partitions = rows, keys = columns
        if (dbg_time)
            fprintf(stderr, "[mat_build_major] nnz=%lld colmajor %.1f ms  rowmajor %.1f ms\n", (long long)nnz,
                    std::chrono::duration<double, std::milli>(tb1 - tb0).count(),
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tb1).count());
    } catch (...) {
        // streams, control blocks and whatever slot buffers / tables exist by now (dsa_mat_destroy only looks at them once has_major is set)
        pma_destroy(h->col);
        pma_destroy(h->row);
        throw;
    }
    h->has_major = true;
}

// dynamicsparse(I, J, V): upload + both builds; *rows_out / *cols_out receive the value ranges of the keys
void mat_build_major(dsa_mat* h, const int64_t* I, const int64_t* J, const double* V, int64_t nnz, KeyRange* rows_out = nullptr, KeyRange* cols_out = nullptr) {
    int64_t *dI = nullptr, *dJ = nullptr; double* dV = nullptr;
    const auto tup0 = std::chrono::steady_clock::now();
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
        static const bool dbg_time = dev_env("DSA_DBG_TIME") != nullptr;
        if (dbg_time) fprintf(stderr, "[mat_build_major] upload of %lld triples from caller memory + key scan %.1f ms\n", (long long)nnz,
                              std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tup0).count());
        if (rows_out) *rows_out = rows;
        if (cols_out) *cols_out = cols;
        if (zr || zc) check_key(0);
        auto fit32 = [](const KeyRange& r) { return !g_force_wide && (!r.known() || (key_fits32(r.lo) && key_fits32(r.hi))); };
        mat_build_major_dev(h, dI, dJ, dV, nnz, !fit32(rows), !fit32(cols), rows, cols);
    } catch (...) { pool_free(dI); pool_free(dJ); pool_free(dV); throw; }      // (a failed build has synchronised and destroyed its streams)
    pool_free(dI); pool_free(dJ); pool_free(dV);
}

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

// setindex! on both orientations for ops [0, n)  src/matrix.jl:53-59
void mat_apply_sets(dsa_mat* h, const int64_t* I, const int64_t* J, const double* V, int64_t n) {
    // colmajor[row, col] = val / rowmajor[col, row] = val: the batch-parallel path takes the caller's columns as they are, the other
    // branches below build the op arrays they need
    const OpBatch bc(OP_MPCSC_SET, I, J, V, n), br(OP_MPCSC_SET, J, I, V, n);
    std::vector<Op> oc, orw;
    auto build_ops = [&] {
        if (!oc.empty() || n == 0) return;
        oc.resize((size_t)n); orw.resize((size_t)n);
        for (int64_t k = 0; k < n; ++k) {
            oc[(size_t)k] = make_op(OP_MPCSC_SET, I[k], J[k], V[k]);
            orw[(size_t)k] = make_op(OP_MPCSC_SET, J[k], I[k], V[k]);
        }
    };
    // size(m) after writes [from, to): a write of a nonzero raises it (src/matrix.jl:44-47)
    auto grow_size = [&](int64_t from, int64_t to) {
        for (int64_t k = from; k < to; ++k) if (V[k] != 0.0) { h->m = std::max(h->m, I[k]); h->n = std::max(h->n, J[k]); }
    };
    // Without tombstones an OP_MPCSC_SET cannot fail (the reference's assert / bounds paths of addpartition! need a
    // deleted partition, App. A.6 (3)), so the two orientations can be updated concurrently; otherwise the colmajor
    // batch runs first and the rowmajor batch is cut at the failing op, like the reference's statement order.
    const bool no_tombstones = h->col.view().dense && h->row.view().dense;
    static const bool par = [] { const char* e = dev_env("DSA_PARBATCH"); return !(e && e[0] == '0'); }();
    // With tombstones a write can only fail while it CREATES a partition in the middle of the table (addpartition!(pcsc, prev),
    // src/pcsr.jl:114-146: the two asserts, and the lookup behind a tombstoned tail).  A batch whose partition keys never decrease and start
    // at or behind the last table entry — which must be live — only ever writes to that entry or appends behind it (find() returns the
    // last position, addcolumn! takes its push! branch, src/pcsr.jl:148-154): it cannot fail either, and the two orientations may run side
    // by side.  That is column generation with deletions: new columns get new, larger ids while old ones are deleted (config 5 + deletecolumn!:
    // 445 -> 330 ms).  Anything else with tombstones keeps the reference's statement order below.
    auto cannot_fail = [&](Pma& P, const int64_t* part_keys_of_ops) -> bool {
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
    };
    const bool side_by_side_ok = no_tombstones || (n >= 128 && cannot_fail(h->col, J) && cannot_fail(h->row, I));
    if (par && side_by_side_ok && n >= 128) {
        // batch-parallel rounds per orientation (writes to existing columns with disjoint footprints run concurrently; new
        // columns and anything else fall back to the sequential sequencer inside run_ops_parallel)
        int32_t ec = 0, er = 0;
        static const bool dbg_time = dev_env("DSA_DBG_TIME") != nullptr;
        // the two orientations are independent structures on their own streams: their round / sequencer loops (host-driven)
        // run side by side, the rowmajor one on a helper thread
        const auto t0 = std::chrono::steady_clock::now();
        int64_t dc = 0, dr = 0;
        std::exception_ptr row_exc;
        auto t_row_done = t0;
        const bool side_by_side = h->col.stream != h->row.stream;
        std::thread row_thread;
        if (side_by_side)
            row_thread = std::thread([&] {
                try { bind_device(h->row); dr = run_ops_parallel(h->row, br, &er); t_row_done = std::chrono::steady_clock::now(); }
                catch (...) { row_exc = std::current_exception(); }
            });
        const int64_t rounds0 = h->row.stat_par_rounds;
        try { dc = run_ops_parallel(h->col, bc, &ec); }
        catch (...) { if (row_thread.joinable()) row_thread.join(); throw; }
        const auto t1 = std::chrono::steady_clock::now();
        if (side_by_side) { row_thread.join(); if (row_exc) std::rethrow_exception(row_exc); }
        else dr = run_ops_parallel(h->row, br, &er);
        if (dbg_time)
            fprintf(stderr, "[mat_apply_sets] n=%lld both orientations %.2f ms (colmajor done after %.2f ms, rowmajor after %.2f ms)  colmajor (par %lld seq %lld ext %lld)  "
                    "rowmajor (par %lld seq %lld ext %lld rounds +%lld)\n", (long long)n,
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(),
                    std::chrono::duration<double, std::milli>(t1 - t0).count(), std::chrono::duration<double, std::milli>(t_row_done - t0).count(), (long long)h->col.stat_par_ops,
                    (long long)h->col.stat_seq_ops, (long long)h->col.h_ctl->stat_extends, (long long)h->row.stat_par_ops, (long long)h->row.stat_seq_ops,
                    (long long)h->row.h_ctl->stat_extends, (long long)(h->row.stat_par_rounds - rounds0));
        if (dbg_time)
            fprintf(stderr, "    rowmajor: sequencer launches %lld  stops by reason [0 unplannable %lld, 1 newcol %lld, 2 limits %lld, 3 shifts %lld, 4 semleaf %lld, "
                    "5 window %lld, 6 scan %lld, 7 conflict %lld]\n", (long long)h->row.stat_seq_launches, (long long)h->row.stat_why[0], (long long)h->row.stat_why[1],
                    (long long)h->row.stat_why[2], (long long)h->row.stat_why[3], (long long)h->row.stat_why[4], (long long)h->row.stat_why[5],
                    (long long)h->row.stat_why[6], (long long)h->row.stat_why[7]);
        if (dbg_time && h->row.h_ctl->prof[7] != 0) {      // -DDSA_PROFILE builds only: shader-clock split of the rowmajor sequencer (cumulative)
            const int64_t* q = h->row.h_ctl->prof;
            const double us = 1.0 / 100.0;                   // s_memtime ticks at 100 MHz
            fprintf(stderr, "    rowmajor sequencer profile (cumulative): kernel %.0f us | %lld matrix writes: table lookup %.0f us, %lld new partitions %.0f us, write in partition %.0f us "
                    "[partition end %.0f, find %.0f, insert/shift %.0f, scan+rebalance %.0f (%lld in-block rebalances %.0f us, %lld slots)] | %lld table merges %.0f us\n",
                    q[7] * us, (long long)q[4], q[0] * us, (long long)q[5], q[1] * us, q[2] * us, q[11] * us, q[8] * us, q[9] * us, q[10] * us, (long long)q[13], q[12] * us,
                    (long long)q[14], (long long)q[6], q[3] * us);
        }
        const int64_t done = std::min(dc, dr);
        grow_size(0, std::min(done + 1, n));
        if (ec && er && dr < dc) fail(er, err_text(er));      // both halves failed: the rowmajor half of the EARLIER write comes first
        if (ec) fail(ec, err_text(ec));
        if (er) fail(er, err_text(er));
        return;
    }
    build_ops();
    if (no_tombstones && h->col.stream != h->row.stream) {
        // A small batch (a column or a few that arrive together, a row): the orientation in which its writes fall into MANY
        // partitions takes the local rounds (one wave per op: k_local_rounds), the one in which they share a few partitions — writes
        // into one column are ordered by nature — its sequencer, side by side.  16 writes of a new column: 218 -> ~120 us.
        if (par && n >= 8) {
            std::vector<int64_t> di(I, I + n), dj(J, J + n);
            std::sort(di.begin(), di.end()); std::sort(dj.begin(), dj.end());
            const int64_t ni = std::unique(di.begin(), di.end()) - di.begin(), nj = std::unique(dj.begin(), dj.end()) - dj.begin();
            Pma* rounds = nullptr; Pma* seq = nullptr; const std::vector<Op>* ro = nullptr; const std::vector<Op>* so = nullptr;
            if (ni >= 2 * nj && ni >= 8) { rounds = &h->row; ro = &orw; seq = &h->col; so = &oc; }          // many rows, few columns
            else if (nj >= 2 * ni && nj >= 8) { rounds = &h->col; ro = &oc; seq = &h->row; so = &orw; }     // many columns, few rows
            if (rounds != nullptr) {
                SeqRun rs;
                seq_start(rs, *seq, *so);
                int32_t er = 0;
                int64_t dr = 0;
                try { dr = run_ops_parallel(*rounds, *ro, &er); } catch (...) { while (seq_step(rs)) {} throw; }
                while (seq_step(rs)) {}
                const int64_t done = std::min(dr, rs.applied);
                grow_size(0, std::min(done + 1, n));
                if (rs.err) fail(rs.err, err_text(rs.err));
                if (er) fail(er, err_text(er));
                return;
            }
        }
        SeqRun rc, rr;
        run_ops_pair(h->col, oc, h->row, orw, rc, rr);
        const int64_t done = std::min(rc.applied, rr.applied);
        grow_size(0, std::min(done + 1, n));
        if (rc.err) fail(rc.err, err_text(rc.err));
        if (rr.err) fail(rr.err, err_text(rr.err));
        return;
    }
    // tombstones present: a write that creates a column can fail (src/pcsr.jl:124,132), so the colmajor batch runs first and the
    // rowmajor batch is cut at the failing op, like the reference's statement order — still through the batch-parallel
    // rounds for everything that is plannable (writes to existing columns); new columns take the sequencer's literal path.
    //
    // The state after a FAILED batch is the reference's too (round 6; until then colmajor could hold writes behind the failing one):
    // the reference stops at write k with colmajor holding writes [0, k] when its rowmajor statement threw, [0, k) when the colmajor one
    // did, rowmajor [0, k) either way (src/matrix.jl:43-62).  Colmajor running ahead of rowmajor is only wrong when ROWMAJOR fails, and
    // whether a write fails depends on nothing but the partition table (which ids are tombstones: src/pcsr.jl:114-162).  So when the
    // rowmajor table holds tombstones the first write it will refuse is found up front by replaying the table — not the slots — on the
    // host (TableReplay), and colmajor is not run beyond it.  The device stays the judge: the error code comes from the device, and
    // when the device accepts what the replay predicted to fail the loop simply goes on behind it.
    const bool par_seq = par && n >= 128;
    int64_t pos = 0;
    while (pos < n) {
        const int64_t rem = n - pos;
        int64_t f = n;                                                  // first write the rowmajor table refuses (n: none)
        const Ctl& rc = *h->row.h_ctl;
        if (rem > 1 && rc.nb_partitions != rc.table_len) {
            TableReplay tr;
            tr.load(h->row);
            for (int64_t k = pos; k < n; ++k) if (tr.touch(I[k]) != 0) { f = k; break; }
        }
        const int64_t end = std::min(n, f + 1);
        std::vector<Op> pc(oc.begin() + pos, oc.begin() + end), pr(orw.begin() + pos, orw.begin() + end);
        int32_t err = 0;
        const int64_t done = (par_seq ? run_ops_parallel(h->col, pc, &err, true) : run_ops(h->col, pc, &err)) + pos;
        if (err) {
            // colmajor refused write `done` (<= f): rowmajor gets the writes in front of it — none of which its table refuses
            pr.resize((size_t)(done - pos));
            int32_t e2 = 0;
            const int64_t d2 = (par_seq ? run_ops_parallel(h->row, pr, &e2, true) : run_ops(h->row, pr, &e2)) + pos;
            // Which write fails FIRST in the reference's order (colmajor then rowmajor of write 0, of write 1, ...): the rowmajor half of an
            // earlier write d2 < done comes before the colmajor half of write `done`.  (Rounds 1-4 reported the colmajor error regardless:
            // tools/fuzz.py run_tombstones seed 503707, EBOUNDS where the reference throws the AssertionError of src/pcsr.jl:132 three writes earlier.)
            const int64_t fail_at = e2 ? d2 : done;
            // the failing write had already updated size(m) in the reference (src/matrix.jl:44-47)
            grow_size(0, std::min(fail_at + 1, n));
            if (e2) fail(e2, err_text(e2));
            fail(err, err_text(err));
        }
        int32_t e2 = 0;
        const int64_t d2 = (par_seq ? run_ops_parallel(h->row, pr, &e2, true) : run_ops(h->row, pr, &e2)) + pos;
        if (e2) {
            grow_size(0, std::min(d2 + 1, n));
            fail(e2, err_text(e2));
        }
        grow_size(pos, end);
        pos = end;
    }
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

void mat_prefetch_spmv_meta(dsa_mat* h) {
    if (!h->has_major) return;
    prefetch_spmv_meta(h->row);
    prefetch_spmv_meta(h->col);
}

// every C-ABI entry that can change a value or a slot of the matrix: the SpMV plans of both orientations are stale from here on
void mat_content_changed(dsa_mat_t* h) {
    for (Pma* P : {&h->col, &h->row}) { ++P->content_epoch; spmv_plan_drop(*P); }
}

}  // namespace

// what sparsex_host.hip calls as well (declared in host.h)
namespace dsa {
namespace host {

void mat_flush(dsa_mat_t* h) {
    if (h->has_major) bind_device(h->col);
    if (h->pi.empty()) return;
    std::vector<int64_t> i, j; std::vector<double> v;
    i.swap(h->pi); j.swap(h->pj); v.swap(h->pv);       // the queue is empty even if the apply fails
    mat_apply_sets(h, i.data(), j.data(), v.data(), (int64_t)i.size());
    mat_prefetch_spmv_meta(h);
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

// both builds of a fresh handle from triples in HBM with known key ranges (ingest_host.hip), then the SpMV meta prefetch every
// constructor ends with
void mat_build_from_dev(dsa_mat* h, const int64_t* dI, const int64_t* dJ, const double* dV, int64_t nnz, KeyRange rows, KeyRange cols) {
    auto fit32 = [](const KeyRange& r) { return !g_force_wide && (!r.known() || (key_fits32(r.lo) && key_fits32(r.hi))); };
    mat_build_major_dev(h, dI, dJ, dV, nnz, !fit32(rows), !fit32(cols), rows, cols);
    try { mat_prefetch_spmv_meta(h); } catch (...) { pma_destroy(h->col); pma_destroy(h->row); h->has_major = false; throw; }
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
    static const bool dbg_time = dev_env("DSA_DBG_TIME") != nullptr;
    const auto ts0 = std::chrono::steady_clock::now();
    const DevView dv = view_dev(S, key);
    const auto ts1 = std::chrono::steady_clock::now();
    if (dv.cnt <= 0) { _check_status(dsa_vec_create(nullptr, nullptr, 0, DSA_COMBINE_ADD, 0, out)); return DSA_OK; }      // PackedMemoryArray(L, T)  src/pcsr.jl:288
    *out = vec_from_packed_dev(S, dv.cnt, std::max<int64_t>(dv.last_key, 0));          // _guess_length(pma)  src/vector.jl:7-8
    if (dbg_time) fprintf(stderr, "[slice] %lld cells: view %.1f us, new vector %.1f us\n", (long long)dv.cnt,
                          std::chrono::duration<double, std::micro>(ts1 - ts0).count(), std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - ts1).count());
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
    try { mat_build_major(h, I, J, V, nnz, &rows, &cols); mat_prefetch_spmv_meta(h); } catch (...) { pma_destroy(h->col); pma_destroy(h->row); delete h; throw; }
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
        try { mat_build_major(h, nullptr, nullptr, nullptr, 0); } catch (...) { pma_destroy(h->col); pma_destroy(h->row); delete h; throw; }
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
    // get_rowids_colids_vals (src/buffer.jl:33-50) is a no-op here: the triples already sit in HBM; only the last partial
    // chunk is still in pinned memory
    FillBuffer& b = h->buf;
    int64_t nnz = 0;
    bool wr = false, wc = false;
    static const bool dbg_time = dev_env("DSA_DBG_TIME") != nullptr;
    const auto tc0 = std::chrono::steady_clock::now();
    // value ranges of everything appended (K-build's composite, the storage width of the keys): every uploaded piece was folded into
    // five running words on the device (k_minmax_acc) — they come back with the wait for the last piece; the appends themselves never
    // look at a key twice
    KeyRange rows, cols;
    if (b.stream) {
        fill_upload_chunk(b);
        HIPCHK(hipMemcpyAsync(b.h_acc, b.d_acc, 5 * sizeof(long long), hipMemcpyDeviceToHost, b.stream));
        HIPCHK(hipStreamSynchronize(b.stream));
        nnz = b.dlen;
        if (nnz > 0) {
            rows.lo = b.h_acc[0]; rows.hi = b.h_acc[1]; cols.lo = b.h_acc[2]; cols.hi = b.h_acc[3];
            wr = g_force_wide || !(key_fits32(rows.lo) && key_fits32(rows.hi));
            wc = g_force_wide || !(key_fits32(cols.lo) && key_fits32(cols.hi));
        }
    }
    // a failed build (out of memory, a HIP error) leaves the matrix what it was: in fill mode, with all of its triples — the
    // builder only reads them — so the caller may free memory and close again, or keep appending
    const auto tc1 = std::chrono::steady_clock::now();
    mat_build_major_dev(h, b.dI, b.dJ, b.dV, nnz, wr, wc, rows, cols);
    const auto tc2 = std::chrono::steady_clock::now();
    h->fillmode = false;
    fill_release(h->buf);
    mat_prefetch_spmv_meta(h);
    if (dbg_time) {
        auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b2) { return std::chrono::duration<double, std::milli>(b2 - a).count(); };
        fprintf(stderr, "[closefillmode] last chunk %.2f ms  build %.2f ms  release + prefetch %.2f ms\n", ms(tc0, tc1), ms(tc1, tc2), ms(tc2, std::chrono::steady_clock::now()));
    }
    API_CATCH
}

int32_t dsa_mat_deletecolumn(dsa_mat_t* h, int64_t col) {      // src/matrix.jl:95-102
    API_TRY
    mat_flush(h);
    if (h->fillmode) fail(DSA_EMODE, "Cannot delete a column in fill mode");
    mat_content_changed(h);
    static const bool dbg_time = dev_env("DSA_DBG_TIME") != nullptr;
    const auto td0 = std::chrono::steady_clock::now();
    std::vector<int64_t> rows; std::vector<double> vals;
    col_view_of(h->col, col, rows, vals);
    const auto td1 = std::chrono::steady_clock::now();
    std::vector<Op> ops;
    for (int64_t r : rows) ops.push_back(make_op(OP_MPCSC_SET, col, r, 0.0));     // rowmajor[col, row] = 0
    std::vector<Op> del{make_op(OP_MPCSC_DELETECOLUMN, 0, col, 0.0)};
    struct Report { bool on; std::chrono::steady_clock::time_point a, b; size_t n; ~Report() { if (on) fprintf(stderr, "[deletecolumn] view %.1f us, %zu twin deletes + deletepartition %.1f us\n",
        std::chrono::duration<double, std::micro>(b - a).count(), n, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - b).count()); } } report{dbg_time, td0, td1, rows.size()};
    // the element deletes of the twin cannot fail and touch the other structure: the deletepartition! of the own orientation is launched
    // on its sequencer, the twin's deletes — different partitions, mostly disjoint footprints — go through the local rounds meanwhile
    // (one wave per op instead of one op after the other: 105 -> 60 us for a column of 16)
    if (h->col.stream != h->row.stream && !ops.empty()) {
        SeqRun rc;
        seq_start(rc, h->col, del);
        int32_t er = 0;
        try { run_ops_parallel(h->row, ops, &er); } catch (...) { while (seq_step(rc)) {} throw; }
        while (seq_step(rc)) {}
        if (er) fail(er, err_text(er));
        if (rc.err) fail(rc.err, err_text(rc.err));
    } else if (h->col.stream != h->row.stream) {
        SeqRun rr, rc;
        run_ops_pair(h->row, ops, h->col, del, rr, rc);
        if (rr.err) fail(rr.err, err_text(rr.err));
        if (rc.err) fail(rc.err, err_text(rc.err));
    } else {
        int32_t err = 0;
        run_ops(h->row, ops, &err);
        if (err) fail(err, err_text(err));
        run_ops(h->col, del, &err);
        if (err) fail(err, err_text(err));
    }
    API_CATCH
}
int32_t dsa_mat_deleterow(dsa_mat_t* h, int64_t row) {         // src/matrix.jl:104-111
    API_TRY
    mat_flush(h);
    if (h->fillmode) fail(DSA_EMODE, "Cannot delete a row in fill mode");
    mat_content_changed(h);
    std::vector<int64_t> cols; std::vector<double> vals;
    col_view_of(h->row, row, cols, vals);
    std::vector<Op> ops;
    for (int64_t c : cols) ops.push_back(make_op(OP_MPCSC_SET, row, c, 0.0));     // colmajor[row, col] = 0
    std::vector<Op> del{make_op(OP_MPCSC_DELETECOLUMN, 0, row, 0.0)};
    if (h->col.stream != h->row.stream && !ops.empty()) {       // (as in deletecolumn!)
        SeqRun rr;
        seq_start(rr, h->row, del);
        int32_t ec = 0;
        try { run_ops_parallel(h->col, ops, &ec); } catch (...) { while (seq_step(rr)) {} throw; }
        while (seq_step(rr)) {}
        if (ec) fail(ec, err_text(ec));
        if (rr.err) fail(rr.err, err_text(rr.err));
    } else if (h->col.stream != h->row.stream) {
        SeqRun rc, rr;
        run_ops_pair(h->col, ops, h->row, del, rc, rr);
        if (rc.err) fail(rc.err, err_text(rc.err));
        if (rr.err) fail(rr.err, err_text(rr.err));
    } else {
        int32_t err = 0;
        run_ops(h->col, ops, &err);
        if (err) fail(err, err_text(err));
        run_ops(h->row, del, &err);
        if (err) fail(err, err_text(err));
    }
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

// ---- reductions per row / column and the in-place scaling D_r A D_c (scale.hip).  Reduce is read-only; scale changes values: both
// SpMV plans are dropped before the first write
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
int32_t dsa_mat_scale_dev(dsa_mat_t* h, double alpha, const double* d_r, int64_t nr, const double* d_c, int64_t nc) {
    API_TRY
    scale_prepare(h, d_r, nr, d_c, nc);
    mat_content_changed(h);
    scale_apply(h, alpha, d_r, d_c);
    mat_prefetch_spmv_meta(h);
    API_CATCH
}
int32_t dsa_mat_scale(dsa_mat_t* h, double alpha, const double* r, int64_t nr, const double* c, int64_t nc) {
    API_TRY
    ScaleStaging st(h, r, nr, c, nc);
    scale_prepare(h, st.d_r, nr, st.d_c, nc);
    mat_content_changed(h);
    scale_apply(h, alpha, st.d_r, st.d_c);
    mat_prefetch_spmv_meta(h);
    HIPCHK(hipStreamSynchronize(h->col.stream));
    HIPCHK(hipStreamSynchronize(h->row.stream));
    API_CATCH
}

// ---- batched delete (delbatch.hip): every column (row) of a key list leaves both orientations in one device pass.  The validate
// pass is in front of the epoch bump: an error leaves layouts and cached plans as they were
int32_t dsa_mat_delete_batch_dev(dsa_mat_t* h, int32_t orientation, const int64_t* d_keys, int64_t n, int64_t* removed_out) {
    API_TRY
    if (removed_out) *removed_out = 0;
    const int64_t cells = delete_batch_prepare(h, orientation, d_keys, n);
    if (cells >= 0) {
        mat_content_changed(h);
        delete_batch_apply(h, orientation, n, cells);
        mat_prefetch_spmv_meta(h);
        if (removed_out) *removed_out = cells;
    }
    API_CATCH
}
int32_t dsa_mat_delete_batch(dsa_mat_t* h, int32_t orientation, const int64_t* keys, int64_t n, int64_t* removed_out) {
    API_TRY
    if (removed_out) *removed_out = 0;
    mat_flush(h);
    if (h->fillmode || !h->has_major) fail(DSA_EMODE, "Cannot delete columns or rows in fill mode");
    Pma& P = orient(h, orientation);
    if (n < 0) fail(DSA_EARG, "delete batch: n is negative");
    if (n > 0 && !keys) fail(DSA_EARG, "delete batch: the key list is NULL");
    if (n > 0) {
        DevStaging b(P.stream);                           // drains the own stream before the keys go back to the pool
        HIPCHK(pool_alloc(&b.p[0], (size_t)n * sizeof(int64_t)));
        HIPCHK(hipMemcpyAsync(b.p[0], keys, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, P.stream));
        const int64_t cells = delete_batch_prepare(h, orientation, static_cast<const int64_t*>(b.p[0]), n);
        mat_content_changed(h);
        delete_batch_apply(h, orientation, n, cells);     // (returns with both streams drained: the twin is done with the table)
        mat_prefetch_spmv_meta(h);
        if (removed_out) *removed_out = cells;
    }
    API_CATCH
}

// ---- dropzeros! / droptol! (droptol.hip): every small cell leaves both orientations in place.  The decide pass is in front of the
// epoch bump: an error, a call that drops nothing and the count-only call leave layouts and cached plans as they were
namespace {
void mat_droptol(dsa_mat_t* h, double tol, const double* d_rtol, int64_t nr, const double* d_ctol, int64_t nc, int32_t count_only,
                 int64_t* dropped_out) {
    const int64_t count = droptol_prepare(h, tol, d_rtol, nr, d_ctol, nc);
    if (count > 0 && !count_only) {
        mat_content_changed(h);
        droptol_apply(h, count);
        mat_prefetch_spmv_meta(h);
    }
    if (dropped_out) *dropped_out = count;
}
}  // namespace
int32_t dsa_mat_droptol_dev(dsa_mat_t* h, double tol, const double* d_rtol, int64_t nr, const double* d_ctol, int64_t nc, int32_t count_only,
                            int64_t* dropped_out) {
    API_TRY
    if (dropped_out) *dropped_out = 0;
    mat_droptol(h, tol, d_rtol, nr, d_ctol, nc, count_only, dropped_out);
    API_CATCH
}
int32_t dsa_mat_droptol(dsa_mat_t* h, double tol, const double* rtol, int64_t nr, const double* ctol, int64_t nc, int32_t count_only,
                        int64_t* dropped_out) {
    API_TRY
    if (dropped_out) *dropped_out = 0;
    ScaleStaging st(h, rtol, nr, ctol, nc);               // flush, DSA_EMODE / DSA_EARG, the vectors in HBM until both streams have drained
    mat_droptol(h, tol, st.d_r, nr, st.d_c, nc, count_only, dropped_out);
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
