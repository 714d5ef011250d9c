// csrc/host.h — what the host units of libdsa_hip.so share (dsa_host.hip and the *_host.hip engine units): the error and launch
// checks, the roctx range of an ABI entry point, the Pma engine struct with the declarations of the engine functions that cross a
// unit boundary, and the handle structs.  The host units are dsa_host.hip, fill_host.hip, matwrite_host.hip, pma_host.hip,
// writes_host.hip, build_host.hip, spmv_host.hip, spmm_host.hip, selprod_host.hip, spgemm_host.hip, mutate_host.hip, scale_host.hip, delbatch_host.hip, droptol_host.hip, update_host.hip, insert_host.hip, assemble_host.hip, sparsex_host.hip, vecops_host.hip, export_host.hip, ingest_host.hip, combine_host.hip and raw_host.hip.  Host units only: a kernel unit
// (rebalance.hip, spmv.hip, sequencer.hip, ...) never includes it; what kernel units share is in dsa_dev.h, find_dev.h, wave_dev.h,
// seq_dev.h, export_dev.h and spmm_dev.h.  Everything declared here lives in dsa::host with hidden visibility — none of it is part of the shared object's
// dynamic symbol table (the definitions in the units inherit the visibility of their declaration here).
#pragma once
#include "../../include/dsa.h"
#include "dsa_dev.h"

#include <chrono>
#include <cstdint>
#include <exception>
#include <string>
#include <unordered_set>
#include <vector>

#pragma GCC visibility push(hidden)
namespace dsa {
namespace host {

struct Fail { int32_t code; std::string msg; long long op = -1; };
[[noreturn]] inline void fail(int32_t code, const std::string& msg) { throw Fail{code, msg}; }
// a failure whose message names op `op` of the batch the callee was given, as op_text(op): a caller that handed on a batch it derived
// (assemble_host.hip) puts the op of ITS caller's batch in its place
inline std::string op_text(unsigned long long k) { return "op " + std::to_string(k) + " (0-based)"; }
[[noreturn]] inline void fail_op(int32_t code, unsigned long long op, const std::string& msg) { throw Fail{code, msg, (long long)op}; }

#define HIPCHK(expr)                                                                               \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) fail(DSA_EHIP, std::string(#expr) + ": " + hipGetErrorString(_e));   \
    } while (0)

// the one check behind a launch_* call: throws Fail{DSA_EHIP, text + hipGetErrorString}
inline void launch_check(hipError_t e, const char* text) {
    if (e != hipSuccess) fail(DSA_EHIP, std::string(text) + hipGetErrorString(e));
}
#define LAUNCH(what, call) launch_check((call), what " launch: ")

// roctx ranges around every ABI entry point; the loader (DSA_ROCTX=1) is in dsa_host.hip
struct Roctx {
    int (*push)(const char*) = nullptr;
    int (*pop)() = nullptr;
    Roctx();
};
const Roctx& roctx();
struct ApiRange {
    bool on;
    explicit ApiRange(const char* name) : on(roctx().push != nullptr) { if (on) roctx().push(name); }
    ~ApiRange() { if (on) roctx().pop(); }
};

#define API_TRY ApiRange _api_range(__func__); try {
#define API_CATCH                                                              \
    } catch (const Fail& f) { ::dsa::set_last_error(f.msg.c_str()); return f.code;    \
    } catch (const std::bad_alloc&) { ::dsa::set_last_error("host allocation failed"); return DSA_EHIP; \
    } catch (const std::exception& e) { ::dsa::set_last_error(e.what()); return DSA_EASSERT; } \
    return DSA_OK;

extern int g_device;                      // the device new handles are created on (dsa_set_device)
extern const int g_wait_policy_default;   // default of Pma::wait_policy (DSA_WAIT_POLICY=1: yield-friendly waits for every new handle)
extern const bool g_force_wide;           // dev knob: DSA_KEYS_WIDE=1 keeps every structure in 64-bit keys

// the timing lines on stderr (development switch DSA_DBG_TIME) and the clock they are taken with: elapsed time from a to b (default:
// to now) in milliseconds / microseconds
inline bool dbg_time() { static const bool on = dev_env("DSA_DBG_TIME") != nullptr; return on; }
using Clock = std::chrono::steady_clock;
inline double elapsed_ms(Clock::time_point a, Clock::time_point b = Clock::now()) { return std::chrono::duration<double, std::milli>(b - a).count(); }
inline double elapsed_us(Clock::time_point a, Clock::time_point b = Clock::now()) { return std::chrono::duration<double, std::micro>(b - a).count(); }

// What an export keeps on its orientation (export_host.hip): a pooled device scratch, grown on demand, and the pinned words its
// kernels hand their results to, allocated at the first export.  Sequence numbers start at 1.
struct ExportArea {
    void* scratch = nullptr; size_t bytes = 0;
    unsigned long long* pin = nullptr; unsigned long long seq = 0;
    void ensure(hipStream_t stream, size_t need, int words);      // at least `need` bytes of scratch (waits for `stream` before it lets go of a smaller one) and `words` pinned words
    unsigned long long next() { return ++seq; }
    void release();
};

// Pooled device staging of a host-form entry point: up to four blocks, released once the stream has drained (also on an error
// after a launch).  Every copy is enqueued on `s`; the caller decides where it waits (sync).
struct DevStaging {
    hipStream_t s; void* p[4] = {nullptr, nullptr, nullptr, nullptr};
    explicit DevStaging(hipStream_t stream) : s(stream) {}
    DevStaging(const DevStaging&) = delete;
    ~DevStaging() { if (p[0] || p[1] || p[2] || p[3]) { (void)hipStreamSynchronize(s); for (void* q : p) pool_free(q); } }
    template <typename T = void> T* at(int q) const { return static_cast<T*>(p[q]); }
    template <typename T = void> T* alloc(int q, size_t bytes) { HIPCHK(pool_alloc(&p[q], bytes)); return at<T>(q); }
    // host -> device and device -> host; `dev` is a block or a place inside one
    void up(void* dev, const void* src, size_t bytes) { HIPCHK(hipMemcpyAsync(dev, src, bytes, hipMemcpyHostToDevice, s)); }
    void down(void* dst, const void* dev, size_t bytes) { HIPCHK(hipMemcpyAsync(dst, dev, bytes, hipMemcpyDeviceToHost, s)); }
    template <typename T = void> T* upload(int q, const void* src, size_t bytes) { alloc(q, bytes); up(p[q], src, bytes); return at<T>(q); }
    // `rows` rows of `row` bytes between block q, where they are packed, and host memory, where they are `pitch` bytes apart
    template <typename T = void> T* upload_rows(int q, const void* src, size_t pitch, size_t row, size_t rows) {
        alloc(q, rows * row);
        HIPCHK(hipMemcpy2DAsync(p[q], row, src, pitch, row, rows, hipMemcpyHostToDevice, s));
        return at<T>(q);
    }
    void down_rows(void* dst, size_t pitch, int q, size_t row, size_t rows) {
        HIPCHK(hipMemcpy2DAsync(dst, pitch, p[q], row, row, rows, hipMemcpyDeviceToHost, s));
    }
    void sync() { HIPCHK(hipStreamSynchronize(s)); }
};

// ------------------------------------------------------------------------------------------------
// One packed-memory array resident in HBM, optionally with PackedCSC / MappedPackedCSC tables
// ------------------------------------------------------------------------------------------------
struct Pma {
    hipStream_t stream = nullptr;
    bool own_stream = false;
    void* keys[2] = {nullptr, nullptr};      // physical key arrays: int32_t unless `wide` (KeyArr, dsa_dev.h)
    bool wide = false;
    double* vals[2] = {nullptr, nullptr};
    uint64_t* occ[2] = {nullptr, nullptr};
    int cur = 0;
    int64_t stat_why[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int64_t cap_alloc = 0;        // slots allocated per buffer
    int64_t occ_words = 0;        // words allocated per bitmap (whole 64-word tiles)
    int64_t occ_dirty[2] = {0, 0}; // high-water mark: words >= occ_dirty[b] of bitmap b are known to be zero
    bool has_sems = false, has_cols = false;
    int64_t* sems = nullptr; int64_t* col_keys = nullptr; uint8_t* col_live = nullptr;
    Ctl* d_ctl = nullptr;
    Ctl* h_ctl = nullptr;         // pinned host mirror
    RebalanceWork work{nullptr, nullptr, 0};
    RebalanceWork work2{nullptr, nullptr, 0};   // second prefix table of K-permute (old and new bitmap)
    uint64_t* occ_old = nullptr;                // bitmap saved by the sequencer at the start of an append run
    Op* run_cells = nullptr; uint64_t* run_flags = nullptr; int64_t* run_out = nullptr; int64_t run_cap = 0;   // cell stream of a MappedPackedCSC append run
    uint64_t* run_memo = nullptr;               // the append replay's memo between runs (appendrun.hip: k_append_run)
    Op* d_ops = nullptr; int64_t ops_cap = 0;
    int wait_policy = g_wait_policy_default;      // how blocking calls wait for a hand-over: 0 spin on the pinned word, 1 block in hipStreamSynchronize first (dsa_*_set_wait_policy)
    uint64_t* d_breaks = nullptr; bool breaks_valid = false;      // run-break bitmap of the ops in d_ops (sequencer.hip: k_op_breaks)
    int64_t* d_opsrc = nullptr; int64_t opsrc_cap = 0;            // the caller's columns of a batch (a, b, v: 3 x opsrc_cap x 8 B) before k_make_ops expands them
    double* d_q = nullptr; int64_t q_cap = 0;      // scratch for lookups (3 arrays of q_cap)
    int32_t* d_err = nullptr;
    int64_t stat_par_rounds = 0, stat_par_ops = 0, stat_seq_ops = 0, stat_seq_launches = 0;      // batch-parallel instrumentation
    int64_t stat_deferred = 0;              // ops a run-ahead round deferred behind a conflict (each is planned again in a later round)
    BurstGraph burst, burst_short;      // cached graphs of a full burst of rounds and of a short one (conflict-heavy phases)
    Plan* d_plans = nullptr; RoundState* d_rs = nullptr; RoundState* h_rs = nullptr;   // batch-parallel writes
    PendOp* d_pend = nullptr;                   // the pending lists of the rounds (2 x ROUND_GMAX: ops deferred behind a conflict, parbatch.hip)
    unsigned long long* h_pub = nullptr; unsigned int pub_seq = 0;      // pinned word k_publish writes the burst number to, and the last number handed out
    DevBufs* d_bufs = nullptr; DevBufs* h_bufs = nullptr;      // the arrays the rounds work on, read from device memory (pinned mirror)
    TableMerge tmerge{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}; int64_t tmerge_cap = 0;   // scratch of the grid-wide table merge (tables.hip)
    int64_t stat_table_merges = 0;
    int64_t stat_grid_rebalances = 0;               // launches of the grid-wide rebalance (window_rebalance / root_rebalance)
    int64_t* d_small = nullptr;                     // 8 x int64 scratch
    int64_t* h_small = nullptr;                     // its pinned host mirror (small read-backs without a pageable staging copy)
    int64_t* h_get = nullptr; unsigned long long get_seq = 0;        // pinned landing area of small lookups (get_batch: keys, partitions, answers, error, sequence number)
    int64_t* h_view = nullptr; unsigned long long view_seq = 0;      // pinned landing area of column views: meta words, sequence number, first cells (col_view_of)
    hipEvent_t ev_handoff = nullptr;      // recorded on `stream` behind work another handle's stream must wait for (a slice built from this structure)
    // bumped by every launch that can move cells or change the tables; SpmvMeta is recomputed when it differs
    int device = 0;              // the device the handle lives on: re-selected at every API entry (a Julia task / finalizer thread or a
                                 // second Python thread calls in with whatever device its thread last selected)
    int64_t layout_epoch = 0;
    int64_t stat_spmv_nomemset = 0;
    // bumped by every C-ABI entry that can change a value or a slot (layout_epoch misses value-only overwrites): the SpMV plan's key
    int64_t content_epoch = 0;
    int64_t stat_spmv_plan = 0, stat_spmv_plan_builds = 0;
    // column-swept SpMV plan of this orientation (spmv.hip: k_spmv_plan), keyed on (content epoch, layout epoch, nx, ny); built on the
    // second product at one key, its usability handed over through h_meta[6..8] (ok, cells, sequence number)
    struct SpmvPlan {
        enum State { NONE, PENDING, USABLE, UNUSABLE } state = NONE;
        int64_t content_epoch = -1, layout_epoch = -1, nx = -1, ny = -1, products = 0;
        PlanDev dev{};
        void* mem[2] = {nullptr, nullptr};      // cells + values, descriptor rows + scratch + row map
        int64_t bytes = 0;
        unsigned long long seq = 0;
    } plan;
    struct SpmvMeta { int64_t epoch = -1; bool ordered = false; int64_t max_extent = 0, max_gap = 0, first_key = 0, last_key = 0; } spmv_meta;
    // its device side: scratch of k_spmv_meta, pinned landing area of the 5 result words, and the epoch a prefetch (enqueued behind
    // the write batch that changed the layout) is in flight for
    unsigned long long* d_meta = nullptr; int64_t* h_meta = nullptr; unsigned long long meta_seq = 0; int64_t meta_inflight_epoch = -1;
    // compressed export (compress.hip): per-tile counts and prefixes; selected export (select.hip): per-key spans, counts and prefixes
    ExportArea cx, sel;
    // submatrix export (submatrix.hip): the key block (hash table of the inner list, spans of the outer list) and the item block
    ExportArea sub, subi;
    // reduce / scale (scale.hip): per-span records, and the pinned {error word, sequence number} of their bounds checks
    ExportArea sc;
    // whole-vector operations (vecops.hip; vectors only): the partials and the scalar of a reduction, the pinned words of vecops.h
    ExportArea vo;
    // batched sparse-x product (spgemm.hip): per-entry spans and per-column counts, and the slabs of the long columns (all zero
    // between two calls)
    ExportArea spg, spgs;
    // batched delete (delbatch.hip): counters, the hash table of the key list and its spans; the pinned words of its two hand-overs
    ExportArea del;
    // dropzeros! / droptol! (droptol.hip): the scale scratch, the counter and the drop masks; the pinned {error word, count, sequence number}
    ExportArea drp;
    // update_values (update.hip): colmajor the resolve records, the claim table, the slots and the winner flags, rowmajor its slots; the
    // pinned words of the one hand-over (colmajor); the event that orders the two streams of a call
    ExportArea upd;
    hipEvent_t ev_upd = nullptr;
    // insert_batch (insert.hip): the sorted ops, their predecessor slots, item counts and prefixes, the tile counts of the array; the
    // pinned words of the orientation's hand-over
    ExportArea ins;
    // assemble (assemble.hip; colmajor only): the sort, the flag words and tile counts, the long-run queue, the folded and the compacted
    // triples, update's miss mask; the pinned {distinct cells, sequence number}; the event that lets the rowmajor stream go on behind
    // the fold and the compaction
    ExportArea asmb;
    hipEvent_t ev_asm = nullptr;
    // combine (combine.hip): the tile arrays, range words and last-semaphore ids of a pass over this orientation; the pinned words of
    // the two roles an operand can have (2 x {error word, four range words, sequence number})
    ExportArea cmb;
    // thresholds  src/pma.jl:58,70,87
    double t_h = 0.7, t_0 = 0.92, p_h = 0.3, p_0 = 0.08, t_d = 0.0, p_d = 0.0;

    int64_t capacity() const { return h_ctl->capacity; }
    KeyArr K() const { return KeyArr{keys[cur], wide ? 1 : 0, 0}; }
    KeyArr KA(int b) const { return KeyArr{keys[b], wide ? 1 : 0, 0}; }
    size_t kb() const { return wide ? sizeof(int64_t) : sizeof(int32_t); }
    double* V() const { return vals[cur]; }
    uint64_t* O() const { return occ[cur]; }
    // what the read-only kernels see (dsa_dev.h: SlotView): the current buffers and the control block's mirror, nothing else
    SlotView view() const {
        const Ctl& c = *h_ctl;
        const uint8_t* live = has_cols ? col_live : nullptr;
        return SlotView{K(), V(), O(), c.capacity, has_sems ? sems : nullptr, has_cols ? col_keys : nullptr, live,
                        c.table_len, c.nb_partitions == c.table_len || live == nullptr};
    }
};

inline void bind_device(const Pma& P) { HIPCHK(hipSetDevice(P.device)); }
inline void check_key(int64_t k) { if (k == 0) fail(DSA_EKEY, "0 is the reserved semaphore key (src/pcsr.jl:23)"); }
inline Op make_op(int32_t kind, int64_t a, int64_t b, double v) { Op o; o.a = a; o.b = b; o.v = v; o.kind = kind; o.pad = 0; return o; }

// A batch of ops as the host hands it to a structure: a ready-made Op array (small batches, mixed kinds), or the caller's COLUMNS —
// op k = (a[k], b ? b[k] : 0, v[k]) of one kind — which go up as they are (16 / 24 bytes per op instead of 32, no Op vector built on
// the host) and are expanded into the op array by a kernel behind the upload (sequencer.hip: k_make_ops).
struct OpBatch {
    int64_t n = 0;
    const Op* ops = nullptr;
    const int64_t* a = nullptr; const int64_t* b = nullptr; const double* v = nullptr; int32_t kind = 0;
    OpBatch() = default;
    OpBatch(const std::vector<Op>& o) : n((int64_t)o.size()), ops(o.data()) {}      // NOLINT: implicit by design
    OpBatch(int32_t kind_, const int64_t* a_, const int64_t* b_, const double* v_, int64_t n_) : n(n_), a(a_), b(b_), v(v_), kind(kind_) {}
    Op at(int64_t k) const {
        if (ops) return ops[k];
        Op o; o.a = a[k]; o.b = b ? b[k] : 0; o.v = v[k]; o.kind = kind; o.pad = 0; return o;
    }
    int64_t key(int64_t k) const { return ops ? ops[k].a : a[k]; }
};

struct SeqRun {
    Pma* P = nullptr;
    const std::vector<Op>* ops = nullptr;
    int64_t n = 0;
    int64_t n_avail = 0;     // ops resident in d_ops (>= n): an append run may consume ops beyond the chunk
    bool active = false;
    int32_t err = 0;         // status of the failing op (0 if none)
    int64_t applied = 0;     // ops fully applied
    int64_t guard = 0;
    bool defer_merge = false; // leave pending table entries to the caller (a batch that goes on with more launches)
};

// view(mpcsc, :, col) that stays in HBM (view_dev): cnt = number of cells, last_key = key of the last one (the largest)
struct DevView { int64_t cnt = 0, last_key = 0; };

// the pinned landing area of views, small packs and small builds: 8 header words (meta [0..4], sequence number [5], written last) + 2 x 1024 cells
constexpr int64_t VIEW_AREA_CELLS = 1024;
// The area is LEASED for one operation and goes back to the pinned pool (pool.hip keeps idle blocks by size class: a lease costs a
// map lookup) when the operation is over: 10^5 small vectors — Coluna keeps that many — would otherwise pin 32 KB each for life.
// The sequence numbers stay per handle and start at 1; the header is zeroed at every lease.  When the operation fails with a kernel
// possibly still in flight the block stays with the handle (released with it) instead of being handed to somebody else.
struct ViewAreaLease {
    Pma& P; int exc;
    explicit ViewAreaLease(Pma& p);
    ~ViewAreaLease();
};

// ---- pma_host.hip: lifecycle, key width, partition tables, geometry, grid rebalances, exports, reads
int64_t capacity_for(int64_t n);
void pma_free_buffers(Pma& P);
void pma_destroy(Pma& P);
void pma_init_common(Pma& P, bool sems, bool cols);
void upload_keys(Pma& P, void* dst, const int64_t* src, int64_t n);
bool keys_fit32(const int64_t* k, int64_t n);
// the storage width a structure needs for keys of this range: 64 bits when an end does not fit 32 (an unknown range fits) or under DSA_KEYS_WIDE=1
inline bool needs_wide(const KeyRange& r) { return g_force_wide || (r.known() && !(key_fits32(r.lo) && key_fits32(r.hi))); }
void widen_keys(Pma& P);
void ensure_tables(Pma& P, int64_t need);
void compute_bounds(Pma& P);
void set_geometry_for_new(Pma& P, int64_t capacity, int64_t nb_elements);
void upload_ctl(Pma& P);
void ensure_capacity_alloc(Pma& P, int64_t slots, bool zero = true);
void root_rebalance(Pma& P, int64_t src_cap, int64_t new_cap, int64_t m, bool src_packed);
void window_rebalance(Pma& P, int64_t ws, int64_t we, int64_t m);
void build_from_packed(Pma& P, const std::vector<int64_t>& keys, const std::vector<double>& vals);
void permute_run(Pma& P, const Op* cells, int64_t i0, int64_t n0);
void wait_policy_block(Pma& P);
void wait_handover(Pma& P, const volatile void* word, uint64_t want, const char* what, uint64_t mask = ~0ull);
void pma_info(Pma& P, int64_t nb_partitions_or_len, int64_t* info);
void export_slots(Pma& P, int64_t* keys, double* vals, uint8_t* occ, int64_t cap);
void export_tables(Pma& P, int64_t* semaphores, int64_t* col_keys, uint8_t* col_live, int64_t table_cap);
void pma_check(Pma& P, int64_t* report);
void get_batch(Pma& P, int mode, const int64_t* qa, const int64_t* qb, int64_t n, double* out);
void read_range(Pma& P, int64_t from, int64_t to, std::vector<int64_t>& ks, std::vector<double>& vs);
void col_view_of(Pma& P, int64_t col, std::vector<int64_t>& ks, std::vector<double>& vs);
DevView view_dev(Pma& P, int64_t col);
int64_t pack_small(Pma& P, KeyArr k, const double* v, const uint64_t* occ, int64_t from, int64_t to, KeyArr ok, double* ov, int64_t out_cap);

// ---- writes_host.hip: the yield loop around the sequencer and the batch-parallel rounds
const char* err_text(int32_t e);
void seq_start(SeqRun& r, Pma& P, const std::vector<Op>& ops);
bool seq_step(SeqRun& r);
int64_t run_ops(Pma& P, const std::vector<Op>& ops, int32_t* err);
int64_t run_ops_parallel(Pma& P, const OpBatch& ops, int32_t* err, bool can_fail = false);
void run_ops_pair(Pma& A, const std::vector<Op>& opsA, Pma& B, const std::vector<Op>& opsB, SeqRun& ra, SeqRun& rb);

// ---- build_host.hip: the bulk build (K-build)
void pma_build_dev(Pma& P, const int64_t* d_part, const int64_t* d_key, const double* d_val, int64_t nnz, int32_t combine,
                   int mode, int64_t nparts_explicit, bool wide, KeyRange part_range = KeyRange(), KeyRange key_range = KeyRange());
bool mat_build_both_dev(Pma& A, Pma& B, const int64_t* d_part, const int64_t* d_key, const double* d_val, int64_t nnz, bool wideA, bool wideB,
                        KeyRange part_range, KeyRange key_range);
void pma_build_from_host(Pma& P, const int64_t* part, const int64_t* key, const double* val, int64_t nnz, int32_t combine,
                         int mode, int64_t nparts_explicit);

// ---- spmv_host.hip: the Pma-level half of the dense product
void spmv_plan_drop(Pma& P);
void prefetch_spmv_meta(Pma& P);
const Pma::SpmvMeta& spmv_meta(Pma& P);
bool spmv_plan_on();
bool spmv_plan_shape_ok(const Pma& P, int64_t nx, int64_t ny);
void spmv_plan_build(Pma& P, int64_t nx, int64_t ny, hipStream_t s);
bool spmv_plan_product(Pma& P, const double* d_x, int64_t nx, double* d_y, int64_t ny, hipStream_t s);

// ---- dsa_host.hip: what sparsex_host.hip and vecops_host.hip need of the handle layer
void ensure_xy(dsa_mat* h, int64_t nx, int64_t ny);
void spmv_dev(dsa_mat* h, int32_t transpose, int32_t algo, const double* d_x, int64_t nx, double* d_y, int64_t ny, hipStream_t s,
              int pattern = 0);
// a vector's queued single writes applied; K-pack of the whole vector into its alternate slot buffer (returns the number of stored
// cells; the cells are still being written on the vector's own stream); the wait of `consumer`'s stream for `producer`'s pack
void vec_flush(dsa_vec* h);
int64_t vec_pack_alt(dsa_vec* h);
void wait_for_pack(dsa_vec* producer, dsa_vec* consumer);

// ---- sparsex_host.hip: the parts of the sparse-x product dsa_mat_mul_vec (vecops_host.hip) runs with x in HBM: the scratch of the
// handle (ny result rows, nx_upload x entries in Spx::dx), the strategy rule, and the product itself enqueued on the walked
// structure's stream (returned); host != nullptr: {count, sequence number, the first pin_cells pairs} go to that pinned area
void spx_ensure(dsa_mat* h, int64_t ny, int64_t nx_upload, hipStream_t s);
bool spx_xdriven(int64_t nx, int64_t ncols);
hipStream_t spx_enqueue(dsa_mat* h, int32_t transpose, bool xdriven, const int64_t* d_xi, const double* d_xv, int64_t nx, int64_t ny, int64_t ncols,
                        int64_t* out_i, double* out_v, int64_t cap, int64_t* d_count, long long* host, unsigned long long seq, int64_t pin_cells);

// ---- matwrite_host.hip: the writes in terms of dsa_mat.  The builds of both orientations of a fresh handle from 1-based int64 triples
// (a constructor hands a handle whose build, or the SpMV meta prefetch behind it, threw to mat_discard: structures and handle go)
void mat_build_major_dev(dsa_mat* h, const int64_t* dI, const int64_t* dJ, const double* dV, int64_t nnz, bool wide_rows, bool wide_cols,
                         KeyRange rows = KeyRange(), KeyRange cols = KeyRange());
void mat_build_major(dsa_mat* h, const int64_t* I, const int64_t* J, const double* V, int64_t nnz, KeyRange* rows_out = nullptr,
                     KeyRange* cols_out = nullptr);
void mat_build_from_dev(dsa_mat* h, const int64_t* dI, const int64_t* dJ, const double* dV, int64_t nnz, KeyRange rows, KeyRange cols);
void mat_discard(dsa_mat* h);
// a batch of setindex! calls, the flush of the queued single writes, what every entry point that changes the matrix does in front of
// its writes and behind them, and deletecolumn! (DSA_COLMAJOR) / deleterow!
void mat_apply_sets(dsa_mat* h, const int64_t* I, const int64_t* J, const double* V, int64_t n);
void mat_flush(dsa_mat* h);
void mat_content_changed(dsa_mat* h);
void mat_prefetch_spmv_meta(dsa_mat* h);
void mat_delete_partition(dsa_mat* h, int32_t orientation, int64_t key);

// ---- ingest_host.hip: a matrix from COO / CSR / CSC arrays in HBM (new handle; the entry points are in dsa_host.hip)
dsa_mat* mat_from_coo_dev(const void* d_I, const void* d_J, const double* d_V, int64_t nnz, int32_t index_bits, int32_t index_base,
                          int64_t m, int64_t n);
dsa_mat* mat_from_compressed_dev(int32_t orientation, int32_t index_bits, int32_t index_base, const void* d_ptr, const void* d_idx,
                                 const double* d_vals, int64_t outer, int64_t inner, int64_t nnz);

// ---- combine_host.hip: alpha * a + beta * b with b's keys shifted by (row_off, col_off), as a new handle of size m x n (< 0: the
// smallest that holds both operands); b may be nullptr (a copy, scaled) or a itself.  The operands are only read.
dsa_mat* mat_combine(dsa_mat* a, double alpha, dsa_mat* b, double beta, int64_t row_off, int64_t col_off, int64_t m, int64_t n);

// ---- spmm_host.hip: the dense multi-vector product (spmm_host: X and Y in host memory, staged packed through HBM)
void spmm_dev(dsa_mat* h, int32_t transpose, const double* d_x, int64_t nx, int64_t k, int64_t ldx, double* d_y, int64_t ny, int64_t ldy,
              hipStream_t s);
void spmm_host(dsa_mat* h, int32_t transpose, const double* x, int64_t nx, int64_t k, int64_t ldx, double* y, int64_t ny, int64_t ldy);

// ---- selprod_host.hip: the product of the partitions of a key list with a dense block (selprod_host: keys, X and Y in host memory)
void selprod_dev(dsa_mat* h, int32_t transpose, const int64_t* d_sel, int64_t nsel, const double* d_x, int64_t nx, int64_t k, int64_t ldx,
                 double* d_y, int64_t ldy, hipStream_t s);
void selprod_host(dsa_mat* h, int32_t transpose, const int64_t* sel, int64_t nsel, const double* x, int64_t nx, int64_t k, int64_t ldx,
                  double* y, int64_t ldy);

// ---- spgemm_host.hip: Y = A S / A' S for k sparse columns, operands and result CSC (d_* are device arrays; *nnz_out also with DSA_ECAP)
void spgemm_csc_dev(dsa_mat* h, int32_t transpose, int32_t index_bits, int32_t index_base, const void* d_xptr, const void* d_xidx,
                    const double* d_xval, int64_t k, int64_t nnzx, void* d_yptr, void* d_yidx, double* d_yval, int64_t cap, int64_t* nnz_out);
void spgemm_csc_host(dsa_mat* h, int32_t transpose, int32_t index_base, const int64_t* xptr, const int64_t* xidx, const double* xval, int64_t k,
                     int64_t* yptr, int64_t* yidx, double* yval, int64_t cap, int64_t* nnz_out);

// ---- export_host.hip: the compressed form of an orientation, of selected columns / rows and of a submatrix (d_* are device arrays; *nnz_out also
// with DSA_ECAP), and the check of an index format that the import shares: index_bits 32 | 64, index_base 0 | 1
void check_index_format(int32_t index_bits, int32_t index_base);
// the verdict on the error word an export, reduce or scale kernel handed over: DSA_EASSERT (value 2 set), DSA_EBOUNDS with the text `outside` (1)
void export_verdict(const unsigned long long* word, const char* what, const char* outside);
void to_compressed_dev(dsa_mat* h, int32_t orientation, int32_t index_bits, int32_t index_base, void* d_ptr, void* d_idx, double* d_vals,
                       int64_t cap, int64_t* nnz_out);
void to_compressed_host(dsa_mat* h, int32_t orientation, int32_t index_base, int64_t* ptr, int64_t* idx, double* vals, int64_t cap,
                        int64_t* nnz_out);
void select_compressed_dev(dsa_mat* h, int32_t orientation, int32_t index_bits, int32_t index_base, const int64_t* d_sel, int64_t nsel,
                           void* d_ptr, void* d_idx, double* d_vals, int64_t cap, int64_t* nnz_out);
void select_compressed_host(dsa_mat* h, int32_t orientation, int32_t index_base, const int64_t* sel, int64_t nsel, int64_t* ptr,
                            int64_t* idx, double* vals, int64_t cap, int64_t* nnz_out);

// A[I, J] (submatrix.hip): the partitions of the outer keys restricted to and renumbered by the inner keys
void submatrix_compressed_dev(dsa_mat* h, int32_t orientation, int32_t index_bits, int32_t index_base, const int64_t* d_outer,
                              int64_t nouter, const int64_t* d_inner, int64_t ninner, void* d_ptr, void* d_idx, double* d_vals,
                              int64_t cap, int64_t* nnz_out);
void submatrix_compressed_host(dsa_mat* h, int32_t orientation, int32_t index_base, const int64_t* outer, int64_t nouter,
                               const int64_t* inner, int64_t ninner, int64_t* ptr, int64_t* idx, double* vals, int64_t cap,
                               int64_t* nnz_out);

// ---- scale_host.hip: per-partition reductions and the in-place scaling D_r A D_c (d_* are device arrays).  A scale is two steps so
// that the entry point can bump the content epoch between them: scale_prepare (flush, checks, the bounds pass over both orientations:
// DSA_EBOUNDS with nothing modified) and scale_apply (the writes, enqueued on both streams).
void reduce_dev(dsa_mat* h, int32_t orientation, int32_t kind, double* d_out, int64_t n_out);
void reduce_host(dsa_mat* h, int32_t orientation, int32_t kind, double* out, int64_t n_out);
bool stream_nt(const Pma& P, int64_t vector_bytes);      // the slot stream of P goes around the cache: it does not fit an XCD's L2 beside the vectors
void scale_prepare(dsa_mat* h, const double* d_r, int64_t nr, const double* d_c, int64_t nc);
void scale_apply(dsa_mat* h, double alpha, const double* d_r, const double* d_c);
void scale_check_args(dsa_mat* h, const double* r, int64_t nr, const double* c, int64_t nc);

// ---- delbatch_host.hip: the batched delete of columns (DSA_COLMAJOR) or rows (DSA_ROWMAJOR), d_keys a device array.  Two steps so
// that the entry point can bump the content epoch between them: delete_batch_prepare (flush, checks, the validate pass: DSA_EMODE /
// DSA_EARG with nothing modified; returns the matrix entries the delete removes, -1 for an empty list) and delete_batch_apply.
int64_t delete_batch_prepare(dsa_mat* h, int32_t orientation, const int64_t* d_keys, int64_t n);
void delete_batch_apply(dsa_mat* h, int32_t orientation, int64_t n, int64_t cells);
// the finish of a pass that only cleared occupancy bits (h_ctl->nb_elements already lowered): the survivors, in slot order, spread over
// [1, capacity] by the root rebalance; a single leaf or an empty array is not moved.  Bumps the layout epoch.
void respread(Pma& X);

// ---- droptol_host.hip: dropzeros! / droptol!, every cell with |v| <= tol, <= d_rtol[row - 1] or <= d_ctol[col - 1] leaves both
// orientations (d_* are device arrays, nullptr = absent).  Two steps so that the entry point can bump the content epoch between them:
// droptol_prepare (flush, checks, the decide pass over both orientations: DSA_EMODE / DSA_EARG / DSA_EBOUNDS / DSA_EASSERT with
// nothing modified; returns the number of cells the predicate drops) and droptol_apply (the marks and root rebalances; returns with
// both control blocks uploaded and both streams drained).
int64_t droptol_prepare(dsa_mat* h, double tol, const double* d_rtol, int64_t nr, const double* d_ctol, int64_t nc);
void droptol_apply(dsa_mat* h, int64_t count);

// ---- update_host.hip: the values of stored cells overwritten (DSA_UPD_SET) or added to (DSA_UPD_ADD) from triples in HBM, and the
// batched read into HBM (d_* are device arrays).  Two steps so that the entry point can bump the content epoch between them:
// update_prepare (flush, checks, locate + claim + resolve over both orientations: DSA_EMODE / DSA_EARG / DSA_EKEY / DSA_EASSERT with
// nothing modified; returns the winning and the missing ops) and update_apply (the stores, enqueued on both streams).
struct UpdateCounts { int64_t updated, missing; };
UpdateCounts update_prepare(dsa_mat* h, int32_t op, int32_t flags, const int64_t* d_I, const int64_t* d_J, const double* d_V, int64_t n,
                            uint8_t* d_missing);
void update_apply(dsa_mat* h, int32_t op, const double* d_V, int64_t n);
void get_batch_dev(dsa_mat* h, const int64_t* d_I, const int64_t* d_J, int64_t n, double* d_out, uint8_t* d_found);
void update_check_args(dsa_mat* h, int32_t op, int32_t flags, const void* I, const void* J, const void* V, int64_t n);

// ---- insert_host.hip: cells that are not stored yet created in both orientations from triples in HBM (d_* are device arrays).  Two
// steps so that the entry point can bump the content epoch between them: insert_prepare (flush, checks, the key scan, then sort +
// locate + verdict over both orientations: DSA_EMODE / DSA_EARG / DSA_EKEY / DSA_EASSERT with nothing modified; returns what the merge
// adds, ops == 0 when there is nothing to insert) and insert_apply (capacity, tables, the merge of both orientations, control blocks
// uploaded, both streams drained).
struct InsertCounts { int64_t ops = 0, existing = 0, items[2] = {0, 0}, parts[2] = {0, 0}; KeyRange rows, cols; };
InsertCounts insert_prepare(dsa_mat* h, const int64_t* d_I, const int64_t* d_J, const double* d_V, int64_t n, int32_t flags, uint8_t* d_existing);
void insert_apply(dsa_mat* h, const InsertCounts& c, const double* d_V, int64_t n);
void insert_check_args(dsa_mat* h, const void* I, const void* J, const void* V, int64_t n, int32_t flags);

// ---- assemble_host.hip: ANY triples in HBM (stored or not, repeated or not) folded to distinct cells on the device, the stored ones
// written by the update, the others created by the insert.  Two steps so that the entry point can bump the content epoch between
// them: assemble_prepare (flush, checks, key scan, sort + fold, update_prepare on the folded cells, then compaction + insert_prepare
// on its misses: every error with nothing modified) and assemble_apply (update_apply, then insert_apply when cells are created).
struct AssembleCounts {
    int64_t distinct = 0, updated = 0, missing = 0;
    InsertCounts ins;
    KeyRange rows, cols;                                                      // of every op: size(m) covers them afterwards, as after setindex!
    const double* folded_V = nullptr; const double* missing_V = nullptr;      // in the scratch: what the two applies store
};
AssembleCounts assemble_prepare(dsa_mat* h, int32_t op, const int64_t* d_I, const int64_t* d_J, const double* d_V, int64_t n);
void assemble_apply(dsa_mat* h, int32_t op, const AssembleCounts& c);
void assemble_check_args(dsa_mat* h, int32_t op, const void* I, const void* J, const void* V, int64_t n);

// Buffer  src/buffer.jl:1-4 — the fill-mode write buffer, DEVICE-RESIDENT: appended triples are staged in two pinned host chunks
// and uploaded asynchronously as a chunk fills (the copy of chunk k overlaps the caller's appends into chunk k+1), so that
// closefillmode! finds the (row, col, value) stream already in HBM and only ships the last partial chunk.  The reference keeps
// a Dict row -> (colids, vals); what it uses the per-row structure for — rejecting a second addrow! of a row id
// (src/buffer.jl:13) — is the `rows` set here; the order of the entries is irrelevant after the (col, row) sort of the
// builder, duplicates of (i, j) are accumulated with + at the flush like the reference (test/functional/sparsematrix.jl:433-437).
struct FillBuffer {
    static constexpr int64_t CHUNK = 1 << 20;            // triples per pinned staging chunk (24 MB)
    static constexpr int64_t EAGER = 1 << 16;            // a finished batch ships its staged triples at once from this many on
    std::vector<uint64_t> row_bits;                       // rows 1 .. 2^28 already written (one bit each, grown on demand)
    std::unordered_set<int64_t> rows_far;                 // ... and the others
    int64_t* hI[2] = {nullptr, nullptr}; int64_t* hJ[2] = {nullptr, nullptr}; double* hV[2] = {nullptr, nullptr};
    hipEvent_t uploaded[2] = {nullptr, nullptr};
    bool in_flight[2] = {false, false};
    static constexpr int64_t PIECE = 1 << 18;            // a chunk goes up in pieces of this many triples, behind the memcpy that stages them
    int cur = 0;
    int64_t fill = 0;                                     // triples in the current pinned chunk
    int64_t sent = 0;                                     // ... of which already on their way to HBM
    int64_t *dI = nullptr, *dJ = nullptr; double* dV = nullptr;
    int64_t dcap = 0, dlen = 0;                           // triples allocated / resident in HBM
    long long* d_acc = nullptr;                           // running value ranges of the resident triples (build.hip: k_minmax_acc), 5 words
    long long* h_acc = nullptr;                           // pinned read-back of them
    hipStream_t stream = nullptr;
    int64_t length = 0;
    int device = 0;
};

// ---- fill_host.hip: the fill-mode buffer.  fill_row_test_and_set: was the row written before; fill_append: addelem! for n entries;
// fill_drain: the last piece goes up and the accumulated words come back (the key ranges only with nnz > 0); fill_release: everything back
bool fill_row_test_and_set(FillBuffer& b, int64_t row);
void fill_append(FillBuffer& b, const int64_t* I, const int64_t* J, const double* V, int64_t n);
struct FillDrain { int64_t nnz = 0; KeyRange rows, cols; };
FillDrain fill_drain(FillBuffer& b);
void fill_release(FillBuffer& b);

}  // namespace host
}  // namespace dsa
#pragma GCC visibility pop

// ---- the handle structs (dsa_host.hip; here for the two groups with entry points of their own: raw_host.hip, sparsex_host.hip)
struct dsa_vec { dsa::host::Pma P; int64_t n = 0; std::vector<int64_t> pk; std::vector<double> pv; };
struct dsa_pcsc { dsa::host::Pma P; };
struct dsa_mat {
    int64_t m = 0, n = 0;
    bool fillmode = false;
    dsa::host::FillBuffer buf;
    bool has_major = false;
    dsa::host::Pma col, row;          // colmajor / rowmajor MappedPackedCSC
    double* d_x = nullptr; double* d_y = nullptr; int64_t x_cap = 0, y_cap = 0;
    // sparse-x product (sparsex.hip): acc / bm keep a ZERO INVARIANT between two products; everything grown, never shrunk
    struct Spx {
        double* acc = nullptr; uint64_t* bm = nullptr; int64_t rows_cap = 0;      // sums per row, one bit per touched row
        uint32_t* tile_cnt = nullptr; uint32_t* tile_off = nullptr; unsigned int* ticket = nullptr; int64_t tiles_cap = 0;
        int64_t* oi = nullptr; double* ov = nullptr; int64_t out_cap = 0;         // packed result in HBM
        int64_t* dx = nullptr; int64_t x_cap = 0;                                 // xi | xv uploaded
        int64_t* d_count = nullptr;
        long long* pin = nullptr;                                                 // landing area: 8 header words + 2 x SPX_PIN_CELLS
        void* stage = nullptr; size_t stage_bytes = 0;                            // pinned staging: x on the way up, long results on the way down
        unsigned long long seq = 0;
        std::vector<hipEvent_t> ev;                                               // behind the pieces of a long result on their way down
        bool dl_started = false; int dl_np = 0; size_t dl_off[8] = {}, dl_bytes[8] = {}; // ... its pieces: offset in [rows | values], bytes
        int64_t res_count = -1;                                                   // result of the last begin (-1: none)
        hipStream_t res_stream = nullptr;
    } spx;
    std::vector<int64_t> pi, pj; std::vector<double> pv;      // queued single writes (non-fill mode)
};
