// csrc/pma_host.hip — one packed-memory array in HBM, host side: the Pma lifecycle (init, alloc, grow, destroy), key width and
// widening, the partition tables, geometry and density bounds, the grid rebalances, the exports and the read paths.
// Host-only unit: launches go through the launch_* functions of the kernel units.
#include "host.h"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>

namespace dsa {
namespace host {

int g_device = 0;
const int g_wait_policy_default = [] { const char* e = getenv("DSA_WAIT_POLICY"); return (e && e[0] == '1') ? 1 : 0; }();

// capacity = 2^ceil(Int, log2(ceil(n / t_h)))   src/pma.jl:64,81,88 (Float64 arithmetic, App. A.1)
int64_t capacity_for(int64_t n) {
    const double c = std::ceil((double)n / 0.7);
    const int64_t e = (int64_t)std::ceil(std::log2(c));
    return (int64_t)1 << e;
}

// the work tables of the grid rebalance and of K-permute, and the saved bitmap of append runs (the caller has synchronised the stream)
static void free_work(Pma& P) {
    pool_free(P.work.tile_cnt); pool_free(P.work.tile_off); pool_free(P.work.status);
    P.work = RebalanceWork{nullptr, nullptr, 0};
    pool_free(P.work2.tile_cnt); pool_free(P.work2.tile_off);
    P.work2 = RebalanceWork{nullptr, nullptr, 0};
    pool_free(P.occ_old);
    P.occ_old = nullptr;
}

void pma_free_buffers(Pma& P) {
    for (int b = 0; b < 2; ++b) {
        pool_free(P.keys[b]); pool_free(P.vals[b]); pool_free(P.occ[b]);     // (the caller has synchronised the stream)
        P.keys[b] = nullptr; P.vals[b] = nullptr; P.occ[b] = nullptr;
    }
    free_work(P);
}

void pma_destroy(Pma& P) {
    if (P.stream) hipStreamSynchronize(P.stream);
    pma_free_buffers(P);
    pool_free(P.sems); pool_free(P.col_keys); pool_free(P.col_live);
    pool_free(P.d_ctl);
    pinned_free(P.h_ctl);
    pool_free(P.d_ops); pool_free(P.d_breaks); pool_free(P.d_opsrc);      // (from the caching allocator since round 5: counted in DSA_INFO_HBM_BYTES)
    if (P.d_q) hipFree(P.d_q);
    pool_free(P.d_err);
    burst_graph_destroy(&P.burst);
    burst_graph_destroy(&P.burst_short);
    if (P.d_plans) hipFree(P.d_plans);
    if (P.d_pend) hipFree(P.d_pend);
    if (P.d_bufs) hipFree(P.d_bufs);
    if (P.h_bufs) hipHostFree(P.h_bufs);
    if (P.d_rs) hipFree(P.d_rs);
    if (P.h_rs) hipHostFree(P.h_rs);
    pool_free(P.d_small);
    pinned_free(P.h_small);
    pinned_free(P.h_view);
    if (P.ev_handoff) (void)hipEventDestroy(P.ev_handoff);
    spmv_plan_drop(P);
    if (P.d_meta) hipFree(P.d_meta);
    pinned_free(P.h_meta);
    P.cx.release();
    P.sel.release();
    P.sub.release();
    P.subi.release();
    P.sc.release();
    P.vo.release();
    P.del.release();
    P.drp.release();
    P.upd.release();
    P.ins.release();
    P.asmb.release();
    if (P.ev_asm) (void)hipEventDestroy(P.ev_asm);
    if (P.ev_upd) (void)hipEventDestroy(P.ev_upd);
    P.cmb.release();
    P.spg.release();
    P.spgs.release();
    if (P.tmerge.sems2) hipFree(P.tmerge.sems2);
    if (P.tmerge.keys2) hipFree(P.tmerge.keys2);
    if (P.tmerge.pkey) hipFree(P.tmerge.pkey);
    if (P.run_cells) hipFree(P.run_cells);
    if (P.run_flags) hipFree(P.run_flags);
    if (P.run_out) hipFree(P.run_out);
    if (P.run_memo) hipFree(P.run_memo);
    if (P.own_stream && P.stream) stream_put(P.stream, P.device);      // synchronised at the top of this function
    P = Pma();
}

// keys cross the host boundary as int64_t; the device array is int32_t unless the structure is wide
void upload_keys(Pma& P, void* dst, const int64_t* src, int64_t n) {
    if (n <= 0) return;
    if (P.wide) { HIPCHK(hipMemcpyAsync(dst, src, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, P.stream)); HIPCHK(hipStreamSynchronize(P.stream)); return; }
    std::vector<int32_t> tmp((size_t)n);
    for (int64_t i = 0; i < n; ++i) tmp[(size_t)i] = (int32_t)src[i];
    HIPCHK(hipMemcpyAsync(dst, tmp.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, P.stream));
    HIPCHK(hipStreamSynchronize(P.stream));
}
static void download_keys(Pma& P, int64_t* dst, const void* src, int64_t n) {      // synchronises the stream
    if (n <= 0) { HIPCHK(hipStreamSynchronize(P.stream)); return; }
    if (P.wide) { HIPCHK(hipMemcpyAsync(dst, src, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost, P.stream)); HIPCHK(hipStreamSynchronize(P.stream)); return; }
    std::vector<int32_t> tmp((size_t)n);
    HIPCHK(hipMemcpyAsync(tmp.data(), src, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, P.stream));
    HIPCHK(hipStreamSynchronize(P.stream));
    for (int64_t i = 0; i < n; ++i) dst[i] = (int64_t)tmp[(size_t)i];
}

// DSA_KEYS_WIDE=1 (A/B measurements, coverage of the wide kernels)
const bool g_force_wide = [] { const char* e = dev_env("DSA_KEYS_WIDE"); return e && e[0] == '1'; }();
bool keys_fit32(const int64_t* k, int64_t n) {
    if (g_force_wide) return false;
    for (int64_t i = 0; i < n; ++i) if (!key_fits32(k[i])) return false;
    return true;
}

static int64_t occ_words_for(int64_t slots) {
    const int64_t w = (slots + 63) / 64;
    return ((w + 63) / 64) * 64;      // whole 64-word tiles (k_tile_count / k_move read lane <-> word)
}

// slot buffers come from the caching allocator (pool.hip): a structure built after another one of the same size was destroyed
// finds its ~100 MB blocks again without a driver call
static void alloc_one_buffer(Pma& P, int b, int64_t slots, bool zero = true) {
    HIPCHK(pool_alloc(&P.keys[b], (size_t)slots * P.kb()));
    HIPCHK(pool_alloc(reinterpret_cast<void**>(&P.vals[b]), (size_t)slots * sizeof(double)));
    const int64_t words = occ_words_for(slots);
    HIPCHK(pool_alloc(reinterpret_cast<void**>(&P.occ[b]), (size_t)words * sizeof(uint64_t)));
    if (zero) HIPCHK(hipMemsetAsync(P.occ[b], 0, (size_t)words * sizeof(uint64_t), P.stream));
}

// zero = false: the caller zeroes the bitmaps and the status table itself (launch_init_fresh: one launch for all of them)
static void alloc_work(Pma& P, int64_t slots, bool zero = true) {
    // (from the caching allocator since round 6: five driver allocations per new structure were a third of what a small vector — a
    //  slice, a filter result — costs to create; the caller has waited for the stream before an existing table is replaced)
    free_work(P);
    P.work.tiles_cap = slots / 4096 + 8;
    HIPCHK(pool_alloc(reinterpret_cast<void**>(&P.work.tile_cnt), (size_t)P.work.tiles_cap * sizeof(uint32_t)));
    HIPCHK(pool_alloc(reinterpret_cast<void**>(&P.work.tile_off), (size_t)P.work.tiles_cap * sizeof(uint32_t)));
    P.work.status_cap = slots / 1024 + slots / (1024 * 64) + 16; P.work.gen = 0;      // one word per 1024-slot tile + one per 64 tiles + the fault word
    HIPCHK(pool_alloc(reinterpret_cast<void**>(&P.work.status), (size_t)P.work.status_cap * sizeof(unsigned long long)));
    if (zero) HIPCHK(hipMemsetAsync(P.work.status, 0, (size_t)P.work.status_cap * sizeof(unsigned long long), P.stream));
    P.work2.tiles_cap = P.work.tiles_cap;
    HIPCHK(pool_alloc(reinterpret_cast<void**>(&P.work2.tile_cnt), (size_t)P.work2.tiles_cap * sizeof(uint32_t)));
    HIPCHK(pool_alloc(reinterpret_cast<void**>(&P.work2.tile_off), (size_t)P.work2.tiles_cap * sizeof(uint32_t)));
    HIPCHK(pool_alloc(reinterpret_cast<void**>(&P.occ_old), (size_t)occ_words_for(slots) * sizeof(uint64_t)));
}

void pma_init_common(Pma& P, bool sems, bool cols) {
    HIPCHK(hipSetDevice(g_device));
    P.device = g_device;
    // stream, control blocks and landing areas come from the caches of pool.hip: a handle is created without a driver call once
    // another one has died (0.5 ms per PMA otherwise: two per matrix, inside every closefillmode! / dynamicsparse)
    HIPCHK(stream_get(&P.stream));
    P.own_stream = true;
    P.has_sems = sems; P.has_cols = cols;
    HIPCHK(pool_alloc(reinterpret_cast<void**>(&P.d_ctl), sizeof(Ctl)));
    HIPCHK(pinned_alloc(reinterpret_cast<void**>(&P.h_ctl), sizeof(Ctl)));
    std::memset(P.h_ctl, 0, sizeof(Ctl));
    HIPCHK(pool_alloc(reinterpret_cast<void**>(&P.d_err), sizeof(int32_t)));
    HIPCHK(pool_alloc(reinterpret_cast<void**>(&P.d_small), 8 * sizeof(int64_t)));
    // one pinned block of 4 KB (the allocator's smallest class) per structure: [0, 64) small read-backs, [64, 72) the word the publish
    // kernels write their number to, [128, 128 + 2 KB) the landing area of small lookups — a structure costs no further pinned blocks
    // (a program with 10^5 small vectors pays 4 KB of pinned memory for each, not 12)
    HIPCHK(pinned_alloc(reinterpret_cast<void**>(&P.h_small), 4096));
    std::memset(P.h_small, 0, 4096);
    P.h_pub = reinterpret_cast<unsigned long long*>(P.h_small + 8);
    P.h_get = P.h_small + 16;
}

void ensure_tables(Pma& P, int64_t need) {
    if (!P.has_sems) return;
    if (need <= P.h_ctl->table_cap) return;
    int64_t ncap = std::max<int64_t>(1024, P.h_ctl->table_cap * (P.h_ctl->table_cap < (1 << 20) ? 4 : 2));      // 4x steps below 1 M entries, 2x above
    while (ncap < need) ncap *= ncap < (1 << 20) ? 4 : 2;
    int64_t* ns = nullptr; int64_t* nk = nullptr; uint8_t* nl = nullptr;
    HIPCHK(pool_alloc(reinterpret_cast<void**>(&ns), (size_t)ncap * sizeof(int64_t)));
    HIPCHK(hipMemsetAsync(ns, 0, (size_t)ncap * sizeof(int64_t), P.stream));
    const int64_t len = P.h_ctl->table_len;
    if (P.sems && len > 0) HIPCHK(hipMemcpyAsync(ns, P.sems, (size_t)len * sizeof(int64_t), hipMemcpyDeviceToDevice, P.stream));
    if (P.has_cols) {
        HIPCHK(pool_alloc(reinterpret_cast<void**>(&nk), (size_t)ncap * sizeof(int64_t)));
        HIPCHK(pool_alloc(reinterpret_cast<void**>(&nl), (size_t)ncap));
        HIPCHK(hipMemsetAsync(nk, 0, (size_t)ncap * sizeof(int64_t), P.stream));
        HIPCHK(hipMemsetAsync(nl, 0, (size_t)ncap, P.stream));
        if (P.col_keys && len > 0) {
            HIPCHK(hipMemcpyAsync(nk, P.col_keys, (size_t)len * sizeof(int64_t), hipMemcpyDeviceToDevice, P.stream));
            HIPCHK(hipMemcpyAsync(nl, P.col_live, (size_t)len, hipMemcpyDeviceToDevice, P.stream));
        }
    }
    // (fresh tables: the memsets above are stream-ordered in front of whatever uses them — no wait; the K-build sizes its tables while
    //  its sort kernels run on this stream, and a wait here would be a wait for the sort)
    if (P.sems || P.col_keys || P.col_live) HIPCHK(hipStreamSynchronize(P.stream));
    pool_free(P.sems); pool_free(P.col_keys); pool_free(P.col_live);
    P.sems = ns; P.col_keys = nk; P.col_live = nl;
    P.h_ctl->table_cap = ncap;
}

// integer density bounds of every level (see Ctl) from the reference's Float64 thresholds
void compute_bounds(Pma& P) {
    Ctl& c = *P.h_ctl;
    if (c.height + 1 > MAX_LEVELS) fail(DSA_EARG, "PMA too tall");
    P.t_d = (P.t_h - P.t_0) / (double)c.height;      // src/pma.jl:47-48,147-148,157-158
    P.p_d = (P.p_h - P.p_0) / (double)c.height;
    for (int64_t h = 0; h <= c.height; ++h) {
        const double W = (double)(c.segment_capacity << h);
        volatile double pm = P.p_d * (double)h;        // separate multiply and add, as Julia evaluates them
        volatile double tm = P.t_d * (double)h;
        const double p = P.p_0 + pm;
        const double t = P.t_0 + tm;
        c.lo[h] = (int64_t)std::ceil(p * W);           // p <= count/W  <=>  count >= ceil(p*W)   (W = 2^k: exact)
        c.hi[h] = (int64_t)std::floor(t * W);          // count/W <= t  <=>  count <= floor(t*W)
    }
}

// _pma geometry  src/pma.jl:42-49
void set_geometry_for_new(Pma& P, int64_t capacity, int64_t nb_elements) {
    Ctl& c = *P.h_ctl;
    const double lc = std::log2((double)capacity);
    const int64_t nb_segs = (int64_t)1 << (int64_t)std::ceil(std::log2((double)capacity / lc));
    c.capacity = capacity;
    c.nb_segments = nb_segs;
    c.segment_capacity = capacity / nb_segs;
    c.height = (int64_t)std::log2((double)nb_segs);
    c.nb_elements = nb_elements;
    compute_bounds(P);
}

void upload_ctl(Pma& P) {
    HIPCHK(hipMemcpyAsync(P.d_ctl, P.h_ctl, sizeof(Ctl), hipMemcpyHostToDevice, P.stream));
    HIPCHK(hipStreamSynchronize(P.stream));   // h_ctl is reused as the download target
}

// grow both slot buffers to at least `slots` (contents of the current buffer are preserved)
void ensure_capacity_alloc(Pma& P, int64_t slots, bool zero) {
    if (slots <= P.cap_alloc) return;
    // growth in steps of 4x (at least 64k slots once the first 4096 are outgrown): a growing array re-allocates its two buffers
    // (13 hipMalloc / hipFree and a stream wait each time) 4 times on the way to 4M slots instead of 10; HBM is not the scarce resource
    // ... up to 2^24 slots; above that the steps are 2x (a structure one slot past a 4x boundary would otherwise hold 4x what it
    // needs twice over: 2^26 + 1 slots -> 2 x 2^28 x 12 B)
    int64_t n = std::max<int64_t>(P.cap_alloc, 4096);
    if (n < slots) n = std::max<int64_t>(n < (1 << 24) ? 4 * n : 2 * n, 65536);
    while (n < slots) n *= n < (1 << 24) ? 4 : 2;
    void* ok[2] = {P.keys[0], P.keys[1]}; double* ov[2] = {P.vals[0], P.vals[1]}; uint64_t* oo[2] = {P.occ[0], P.occ[1]};
    const int64_t old_words = P.occ_words, old_slots = P.cap_alloc;
    for (int b = 0; b < 2; ++b) { P.keys[b] = nullptr; P.vals[b] = nullptr; P.occ[b] = nullptr; }
    for (int b = 0; b < 2; ++b) alloc_one_buffer(P, b, n, zero);
    if (ok[P.cur] != nullptr && old_slots > 0) {
        HIPCHK(hipMemcpyAsync(P.keys[P.cur], ok[P.cur], (size_t)old_slots * P.kb(), hipMemcpyDeviceToDevice, P.stream));
        HIPCHK(hipMemcpyAsync(P.vals[P.cur], ov[P.cur], (size_t)old_slots * sizeof(double), hipMemcpyDeviceToDevice, P.stream));
        HIPCHK(hipMemcpyAsync(P.occ[P.cur], oo[P.cur], (size_t)old_words * sizeof(uint64_t), hipMemcpyDeviceToDevice, P.stream));
    }
    if (ok[0] || ok[1]) HIPCHK(hipStreamSynchronize(P.stream));      // (old buffers: copied out of and about to be freed; a fresh array waits for nobody)
    for (int b = 0; b < 2; ++b) { pool_free(ok[b]); pool_free(ov[b]); pool_free(oo[b]); }
    P.occ_dirty[1 - P.cur] = 0;                       // fresh, zero-filled; occ_dirty[cur] keeps its value
    P.cap_alloc = n;
    P.occ_words = occ_words_for(n);
    alloc_work(P, n, zero);
}

// pack + spread of the whole array into the other buffer: cells of cur[1..src_cap] -> alt[1..new_cap]
// (root _even_rebalance!, _extend!, pack! + _shrink!)  src/pma.jl:94-103,135-161
void root_rebalance(Pma& P, int64_t src_cap, int64_t new_cap, int64_t m, bool src_packed) {
    ++P.stat_grid_rebalances;
    ensure_capacity_alloc(P, std::max(src_cap, new_cap));
    ++P.layout_epoch;
    const int alt = 1 - P.cur;
    LAUNCH("rebalance", launch_rebalance(P.KA(P.cur), P.vals[P.cur], P.occ[P.cur], 1, src_cap, src_packed,
                                         P.KA(alt), P.vals[alt], P.occ[alt], 1, new_cap, m,
                                         P.has_sems ? P.sems : nullptr, &P.work, P.stream));
    // bits beyond the new capacity must be zero in the buffer that becomes current; only the words that
    // may still hold stale bits (below the buffer's high-water mark) are cleared
    const int64_t first_word = (new_cap + 63) / 64;
    if (first_word < P.occ_dirty[alt])
        HIPCHK(hipMemsetAsync(P.occ[alt] + first_word, 0, (size_t)(P.occ_dirty[alt] - first_word) * sizeof(uint64_t), P.stream));
    P.occ_dirty[alt] = first_word;
    P.cur = alt;
}

// an interior window (too wide for the LDS paths): pack! into the alternate buffer, spread! back from there — the two halves of
// _even_rebalance! (src/pma.jl:94-103) as two launches of the same kernel: unpacked source -> m packed cells, packed source ->
// spread window.  (2 W + 2 m) cells of traffic and two launches; round 2 rebalanced into the alternate buffer and copied the
// window back with three device-to-device copies: 4 W cells, four launches.)
void window_rebalance(Pma& P, int64_t ws, int64_t we, int64_t m) {
    if (ws == 1 && we == P.capacity()) { root_rebalance(P, P.capacity(), P.capacity(), m, false); return; }
    const int alt = 1 - P.cur;
    ++P.layout_epoch;
    ++P.stat_grid_rebalances;
    if (m <= 0) {                                     // nothing to move: every slot of the window becomes a gap
        LAUNCH("clear", launch_clear_occ(P.O(), ws, we, P.stream));
        return;
    }
    // pack!: the m cells of [ws, we] -> alt[ws .. ws + m - 1] (no gaps: the destination window has exactly m slots); the semaphore
    // table is not touched (positions in the scratch buffer mean nothing)
    launch_check(launch_rebalance(P.K(), P.V(), P.O(), ws, we, false, P.KA(alt), P.vals[alt], P.occ[alt], ws, ws + m - 1, m,
                                  nullptr, &P.work, P.stream), "rebalance launch (pack): ");
    P.occ_dirty[alt] = std::max<int64_t>(P.occ_dirty[alt], (ws + m - 1 + 63) / 64);      // the scratch bitmap words written by the pack
    // spread!: packed source -> the window in the current buffer, occupancy words and semaphores[] included
    launch_check(launch_rebalance(P.KA(alt), P.vals[alt], P.occ[alt], ws, ws + m - 1, true, P.K(), P.V(), P.O(), ws, we, m,
                                  P.has_sems ? P.sems : nullptr, &P.work, P.stream), "rebalance launch (spread): ");
}

// PackedMemoryArray(keys, values; sort=false) + _pma  src/pma.jl:42-55,69-84 from an already ordered
// cell stream; n == 0 -> PackedMemoryArray(K, T) (capacity for 100 expected cells)  src/pma.jl:86-91
void build_from_packed(Pma& P, const std::vector<int64_t>& keys, const std::vector<double>& vals) {
    const int64_t n = (int64_t)keys.size();
    if (P.cap_alloc == 0) P.wide = !keys_fit32(keys.data(), n);
    const int64_t capacity = capacity_for(n == 0 ? 100 : n);
    set_geometry_for_new(P, capacity, n);
    ensure_capacity_alloc(P, 2 * capacity);
    if (n > 0) {
        upload_keys(P, P.keys[P.cur], keys.data(), n);
        HIPCHK(hipMemcpyAsync(P.V(), vals.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice, P.stream));
    }
    // _even_rebalance!(pma, 1, capacity, n): a no-op when the array is exactly one leaf (src/pma.jl:96-99)
    P.h_ctl->stat_rebalances = 0; P.h_ctl->stat_window_slots = 0;
    if (capacity != P.h_ctl->segment_capacity) { P.h_ctl->stat_rebalances = 1; P.h_ctl->stat_window_slots = capacity; }
    root_rebalance(P, std::max<int64_t>(n, 1), capacity, n, true);
    upload_ctl(P);
}

// An append run was simulated on the bitmap of the current buffer (appendrun.hip): the y_we cells that existed before the
// run (positions: saved bitmap occ_old) followed by the cells cells[i0..] move to the set bits of the current bitmap,
// written into the alternate buffer, which becomes current.
void permute_run(Pma& P, const Op* cells, int64_t i0, int64_t n0) {
    const int alt = 1 - P.cur;
    const int64_t cap = P.capacity();
    ++P.layout_epoch;
    LAUNCH("permute", launch_permute(P.K(), P.V(), P.occ_old, cap, P.KA(alt), P.vals[alt], P.O(), cap, n0, cells, i0,
                                     P.has_sems ? P.sems : nullptr, &P.work, &P.work2, P.stream));
    const int64_t words = (cap + 63) / 64;
    HIPCHK(hipMemcpyAsync(P.occ[alt], P.O(), (size_t)words * sizeof(uint64_t), hipMemcpyDeviceToDevice, P.stream));
    if (words < P.occ_dirty[alt])
        HIPCHK(hipMemsetAsync(P.occ[alt] + words, 0, (size_t)(P.occ_dirty[alt] - words) * sizeof(uint64_t), P.stream));
    P.occ_dirty[alt] = words;
    P.cur = alt;
}

// First key outside Int32: both slot buffers are re-allocated with 64-bit keys, the current one converted on the device.
// (The alternate buffer holds no live data between operations.)
void widen_keys(Pma& P) {
    if (P.wide) return;
    HIPCHK(hipStreamSynchronize(P.stream));
    void* old[2] = {P.keys[0], P.keys[1]};
    for (int b = 0; b < 2; ++b) { P.keys[b] = nullptr; if (P.cap_alloc > 0) HIPCHK(pool_alloc(&P.keys[b], (size_t)P.cap_alloc * sizeof(int64_t))); }
    if (P.cap_alloc > 0 && old[P.cur] != nullptr) {
        LAUNCH("widen", launch_widen_keys(old[P.cur], P.keys[P.cur], P.cap_alloc, P.stream));
        HIPCHK(hipStreamSynchronize(P.stream));
    }
    for (int b = 0; b < 2; ++b) pool_free(old[b]);
    P.wide = true;
}

// Blocking calls wait for a word the last kernel of the launch writes into pinned memory.  Policy 0 polls it (lowest latency; the
// calling thread spins on a host core for the microseconds to milliseconds the device needs).  Policy 1 parks the thread in
// hipStreamSynchronize first — the word is there when it returns — for hosts that run many tasks on few threads (a Julia process
// driving Coluna): the kernels, the hand-over and the results are the same, only the way the host waits differs.
void wait_policy_block(Pma& P) {
    if (P.wait_policy == 1) HIPCHK(hipStreamSynchronize(P.stream));
}
// waits (after the policy's block) for the number `want` in the pinned `word` of a launch on P's stream; `what` names the operation in the error
void wait_handover(Pma& P, const volatile void* word, uint64_t want, const char* what, uint64_t mask) {
    wait_policy_block(P);
    const hipError_t e = wait_pinned_seq(word, want, P.stream, mask);
    if (e == hipErrorUnknown) fail(DSA_EHIP, std::string(what) + ": finished without publishing its result");
    launch_check(e, (std::string(what) + ": ").c_str());
}

void pma_info(Pma& P, int64_t nb_partitions_or_len, int64_t* info) {
    const Ctl& c = *P.h_ctl;
    std::memset(info, 0, sizeof(int64_t) * DSA_INFO_COUNT);
    info[DSA_INFO_CAPACITY] = c.capacity;
    info[DSA_INFO_SEGMENT_CAPACITY] = c.segment_capacity;
    info[DSA_INFO_NB_SEGMENTS] = c.nb_segments;
    info[DSA_INFO_NB_ELEMENTS] = c.nb_elements;
    info[DSA_INFO_HEIGHT] = c.height;
    info[DSA_INFO_NB_PARTITIONS] = nb_partitions_or_len;
    info[DSA_INFO_TABLE_LEN] = c.table_len;
    info[DSA_INFO_STAT_WINDOW_SLOTS] = c.stat_window_slots;
    info[DSA_INFO_STAT_REBALANCES] = c.stat_rebalances;
    info[DSA_INFO_STAT_EXTENDS] = c.stat_extends;
    info[DSA_INFO_STAT_SHRINKS] = c.stat_shrinks;
    info[11] = P.stat_par_rounds; info[12] = P.stat_par_ops; info[13] = P.stat_seq_ops;
    info[DSA_INFO_STAT_SPMV_NOMEMSET] = P.stat_spmv_nomemset;
    info[DSA_INFO_STAT_GRID_REBALANCES] = P.stat_grid_rebalances;
    info[DSA_INFO_STAT_SPMV_PLAN] = P.stat_spmv_plan;
    info[DSA_INFO_STAT_SPMV_PLAN_BUILDS] = P.stat_spmv_plan_builds;
    // HBM held by the structure: both slot buffers (keys, values, bitmap), the saved bitmap of append runs, the tables and the merge scratch
    info[DSA_INFO_HBM_BYTES] = 2 * (P.cap_alloc * (int64_t)(P.kb() + sizeof(double)) + P.occ_words * 8) + (P.occ_old ? P.occ_words * 8 : 0) +
                               (P.has_sems ? c.table_cap * 8 : 0) + (P.has_cols ? c.table_cap * 9 : 0) + 2 * P.tmerge_cap * 8 +
                               (P.d_ops ? P.ops_cap * (int64_t)sizeof(Op) + (P.ops_cap / 64 + 8) * 8 : 0) + (P.d_opsrc ? P.opsrc_cap * 24 : 0) +      // op array, run-break bitmap, batch columns
                               P.plan.bytes +     // the SpMV plan: 12 B per stored cell + descriptor rows + 4 B per partition (row map)
                               (int64_t)P.sel.bytes +     // scratch of the selected export: 32 B per key of the longest selection so far
                               (int64_t)(P.sub.bytes + P.subi.bytes);      // ... of the submatrix export: hash table, spans, work items
}

void export_slots(Pma& P, int64_t* keys, double* vals, uint8_t* occ, int64_t cap) {
    const int64_t c = P.capacity();
    if (cap < c) fail(DSA_ECAP, "output buffers smaller than capacity");
    std::vector<uint64_t> words((size_t)((c + 63) / 64));
    download_keys(P, keys, P.keys[P.cur], c);
    HIPCHK(hipMemcpyAsync(vals, P.V(), (size_t)c * sizeof(double), hipMemcpyDeviceToHost, P.stream));
    HIPCHK(hipMemcpyAsync(words.data(), P.O(), words.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, P.stream));
    HIPCHK(hipStreamSynchronize(P.stream));
    for (int64_t i = 0; i < c; ++i) {
        const uint8_t o = (words[(size_t)(i >> 6)] >> (i & 63)) & 1ull;
        occ[i] = o;
        if (!o) { keys[i] = 0; vals[i] = 0.0; }
    }
}

void export_tables(Pma& P, int64_t* semaphores, int64_t* col_keys, uint8_t* col_live, int64_t table_cap) {
    const int64_t tl = P.h_ctl->table_len;
    if (table_cap < tl) fail(DSA_ECAP, "table buffers too small");
    if (tl == 0) return;
    HIPCHK(hipMemcpyAsync(semaphores, P.sems, (size_t)tl * sizeof(int64_t), hipMemcpyDeviceToHost, P.stream));
    if (col_keys) {
        HIPCHK(hipMemcpyAsync(col_keys, P.col_keys, (size_t)tl * sizeof(int64_t), hipMemcpyDeviceToHost, P.stream));
        HIPCHK(hipMemcpyAsync(col_live, P.col_live, (size_t)tl, hipMemcpyDeviceToHost, P.stream));
    }
    HIPCHK(hipStreamSynchronize(P.stream));
    if (col_keys) for (int64_t i = 0; i < tl; ++i) if (!col_live[i]) col_keys[i] = 0;
}

void pma_check(Pma& P, int64_t* report) {
    unsigned long long* d = nullptr;
    HIPCHK(hipMalloc(&d, 8 * sizeof(unsigned long long)));
    unsigned long long r[8] = {0};
    hipError_t e = launch_check(P.view(), P.occ_words, d, P.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(r, d, sizeof(r), hipMemcpyDeviceToHost, P.stream);
    // no table entry may be pending outside a batch (tables.hip): the DEVICE copy of the counter is the one the kernels trust
    int64_t dev_pending = 0, merge_fault = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&dev_pending, reinterpret_cast<const char*>(P.d_ctl) + offsetof(Ctl, n_pending), sizeof(int64_t), hipMemcpyDeviceToHost, P.stream);
    // the grid-wide table merge raises hdr[2] if it was ever handed more entries than it takes (cannot happen: TABLE_PEND_MAX)
    if (e == hipSuccess && P.tmerge.hdr != nullptr) e = hipMemcpyAsync(&merge_fault, P.tmerge.hdr + 2, sizeof(int64_t), hipMemcpyDeviceToHost, P.stream);
    unsigned long long move_fault = 0;
    if (e == hipSuccess && P.work.status != nullptr)
        e = hipMemcpyAsync(&move_fault, P.work.status + P.work.status_cap - 1, sizeof(move_fault), hipMemcpyDeviceToHost, P.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(P.stream);
    hipFree(d);
    launch_check(e, "check: ");
    if (move_fault != 0) fail(DSA_EHIP, "a rebalance launch gave up waiting for its prefix table (k_move2: dispatch-order assumption violated)");
    for (int i = 0; i < 8; ++i) report[i] = (int64_t)r[i];
    const int64_t live = P.has_sems ? P.h_ctl->nb_partitions : 0;
    report[6] = (report[0] != P.h_ctl->nb_elements || report[1] != live || dev_pending != 0 || P.h_ctl->n_pending != 0 || merge_fault != 0) ? 1 : 0;
}

static void ensure_q(Pma& P, int64_t n) {
    if (n <= P.q_cap) return;
    if (P.d_q) hipFree(P.d_q);
    P.q_cap = std::max<int64_t>(n, 256);
    HIPCHK(hipMalloc(&P.d_q, (size_t)P.q_cap * 3 * sizeof(double)));
}

// batched getindex on the device; mode as in launch_get_batch
void get_batch(Pma& P, int mode, const int64_t* qa, const int64_t* qb, int64_t n, double* out) {
    if (n <= 0) return;
    if (n <= 64) {
        // a scalar getindex or a handful of them: one launch that reads its queries from, and writes its answers to, pinned memory
        for (int64_t i = 0; i < n; ++i) { P.h_get[i] = qa[i]; P.h_get[64 + i] = qb ? qb[i] : 0; }
        const unsigned long long seq = ++P.get_seq;
        __atomic_thread_fence(__ATOMIC_RELEASE);
        LAUNCH("get", launch_get_small(mode, P.view(), P.h_get, (int)n, seq, P.stream));
        wait_handover(P, P.h_get + 193, seq, "get");
        std::memcpy(out, P.h_get + 128, (size_t)n * sizeof(double));
        const int32_t err = (int32_t)P.h_get[192];
        if (err) fail(err, err == DSA_EBOUNDS ? "partition index out of range" : "partition has no semaphore");
        return;
    }
    ensure_q(P, n);
    int64_t* d_qa = reinterpret_cast<int64_t*>(P.d_q);
    int64_t* d_qb = d_qa + P.q_cap;
    double* d_out = P.d_q + 2 * P.q_cap;
    HIPCHK(hipMemcpyAsync(d_qa, qa, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, P.stream));
    if (qb) HIPCHK(hipMemcpyAsync(d_qb, qb, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, P.stream));
    HIPCHK(hipMemsetAsync(P.d_err, 0, sizeof(int32_t), P.stream));
    LAUNCH("get", launch_get_batch(mode, P.view(), d_qa, d_qb, n, d_out, P.d_err, P.stream));
    int32_t err = 0;
    HIPCHK(hipMemcpyAsync(out, d_out, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, P.stream));
    HIPCHK(hipMemcpyAsync(&err, P.d_err, sizeof(int32_t), hipMemcpyDeviceToHost, P.stream));
    HIPCHK(hipStreamSynchronize(P.stream));
    if (err) fail(err, err == DSA_EBOUNDS ? "partition index out of range" : "partition has no semaphore");
}

static void ensure_view_area(Pma& P) {
    if (P.h_view) return;
    HIPCHK(pinned_alloc(reinterpret_cast<void**>(&P.h_view), (size_t)(8 + 2 * VIEW_AREA_CELLS) * sizeof(int64_t)));
    std::memset(P.h_view, 0, 8 * sizeof(int64_t));          // header: a stale sequence number of the block's previous user must not match
}
ViewAreaLease::ViewAreaLease(Pma& p) : P(p), exc(std::uncaught_exceptions()) { ensure_view_area(P); }
ViewAreaLease::~ViewAreaLease() {
    if (std::uncaught_exceptions() > exc) return;
    pinned_free(P.h_view); P.h_view = nullptr;
}

static void read_range_general(Pma& P, int64_t from, int64_t to, std::vector<int64_t>& ks, std::vector<double>& vs) {
    ks.clear(); vs.clear();
    if (to < from) return;
    const int alt = 1 - P.cur;
    int64_t cnt = 0;
    LAUNCH("compact", launch_compact_range(P.K(), P.V(), P.O(), from, to, P.KA(alt), P.vals[alt], P.cap_alloc, &P.work, &cnt, P.stream));
    if (cnt == 0) return;
    ks.resize((size_t)cnt); vs.resize((size_t)cnt);
    HIPCHK(hipMemcpyAsync(vs.data(), P.vals[alt], (size_t)cnt * sizeof(double), hipMemcpyDeviceToHost, P.stream));
    download_keys(P, ks.data(), P.keys[alt], cnt);        // synchronises
}

// range_from > 0: the stored cells of the slot range [range_from, range_to] instead of the column `col` (at most VIEW_SMALL_SLOTS slots)
static void view_small(Pma& P, int64_t col, int64_t range_from, int64_t range_to, std::vector<int64_t>& ks, std::vector<double>& vs) {
    // one launch (partition lookup + K-pack of its slot range into the idle alternate buffer) and one host round trip for
    // partitions of up to VIEW_SMALL_SLOTS slots; the first SPEC cells travel with the meta words, longer views fetch the rest
    constexpr int64_t SPEC = 512;
    ks.clear(); vs.clear();
    const int alt = 1 - P.cur;
    const int64_t out_cap = std::min<int64_t>(P.cap_alloc, VIEW_SMALL_SLOTS);
    const int64_t spec = std::min<int64_t>(SPEC, out_cap);
    int64_t r[5] = {0, 0, 0, 0, 0};
    {
        // the kernel writes the meta words and the first SPEC cells straight into a pinned landing area and then a sequence number: the host
        // polls for it — no copy command, no stream synchronisation (60 -> 20 us per view)
        ViewAreaLease lease(P);
        const unsigned long long seq = ++P.view_seq;
        LAUNCH("view", launch_view_small(P.view(), col, P.KA(alt), P.vals[alt], out_cap, P.d_small, P.h_view, SPEC, seq, range_from, range_to,
                                         P.stream));
        wait_handover(P, P.h_view + 5, seq, "view");
        for (int q = 0; q < 5; ++q) r[q] = P.h_view[q];
        const int64_t have = std::max<int64_t>(0, std::min<int64_t>(r[4], spec));
        ks.assign(P.h_view + 8, P.h_view + 8 + have);
        vs.resize((size_t)have);
        std::memcpy(vs.data(), P.h_view + 8 + SPEC, (size_t)have * sizeof(double));
        ks.resize((size_t)spec); vs.resize((size_t)spec);
    }
    if (r[2] != 0) { ks.clear(); vs.clear(); fail((int32_t)r[2], "partition has no semaphore"); }
    if (r[0] == 0) { ks.clear(); vs.clear(); return; }       // empty view: the column does not exist (src/views.jl:17,24)
    const int64_t cnt = r[4];
    if (cnt < 0) { read_range_general(P, r[0], r[1], ks, vs); return; }   // a long partition: general K-pack path
    ks.resize((size_t)cnt); vs.resize((size_t)cnt);
    if (cnt > spec) {
        HIPCHK(hipMemcpyAsync(vs.data() + spec, P.vals[alt] + spec, (size_t)(cnt - spec) * sizeof(double), hipMemcpyDeviceToHost, P.stream));
        download_keys(P, ks.data() + spec, (char*)P.keys[alt] + (size_t)spec * P.kb(), cnt - spec);
    }
}

// stored cells of the slot range [from, to] in slot order: K-pack on the device into the alternate buffer (free between
// rebalances), then only the packed cells cross PCIe
void read_range(Pma& P, int64_t from, int64_t to, std::vector<int64_t>& ks, std::vector<double>& vs) {
    // up to VIEW_SMALL_SLOTS slots (iteration over a small vector, a short slice): one launch that packs the cells and hands the first 512 to the
    // host through pinned memory (nonzeros() of a 100-entry vector: 80 -> 25 us); longer ranges: tile counts + scan + K-pack
    if (to >= from && from >= 1 && to - from + 1 <= VIEW_SMALL_SLOTS && to - from + 1 <= P.cap_alloc) { view_small(P, 0, from, to, ks, vs); return; }
    read_range_general(P, from, to, ks, vs);
}

void col_view_of(Pma& P, int64_t col, std::vector<int64_t>& ks, std::vector<double>& vs) { view_small(P, col, 0, 0, ks, vs); }

// view(mpcsc, :, col) (src/views.jl:15-35) that stays in HBM: the stored cells of the column packed, in slot order, at the front of
// P's idle alternate buffer (P.KA(1 - P.cur), P.vals[1 - P.cur]); only the meta words reach the host (through the pinned landing area:
// no copy command).  cnt = number of cells, last_key = key of the last one (the largest: a partition is key-ordered).
DevView view_dev(Pma& P, int64_t col) {
    DevView dv;
    const int alt = 1 - P.cur;
    const int64_t out_cap = std::min<int64_t>(P.cap_alloc, VIEW_SMALL_SLOTS);
    int64_t r[6] = {0, 0, 0, 0, 0, 0};
    {   // (the landing area is leased for the hand-over only)
        ViewAreaLease lease(P);
        const unsigned long long seq = ++P.view_seq;
        LAUNCH("view", launch_view_small(P.view(), col, P.KA(alt), P.vals[alt], out_cap, P.d_small, P.h_view, 0, seq, 0, 0, P.stream));
        wait_handover(P, P.h_view + 5, seq, "view");
        for (int q = 0; q < 5; ++q) r[q] = P.h_view[q];
        r[5] = P.h_view[6];
    }
    if (r[2] != 0) fail((int32_t)r[2], "partition has no semaphore");
    if (r[0] == 0) return dv;                                  // the column does not exist (src/views.jl:17,24)
    dv.cnt = r[4]; dv.last_key = r[5];
    if (dv.cnt < 0) {                                          // a long partition: tile counts + scan + K-pack; the count and one key come back
        int64_t cnt = 0;
        LAUNCH("compact", launch_compact_range(P.K(), P.V(), P.O(), r[0], r[1], P.KA(alt), P.vals[alt], P.cap_alloc, &P.work, &cnt, P.stream));
        dv.cnt = cnt; dv.last_key = 0;
        if (cnt > 0) {
            HIPCHK(hipMemcpyAsync(P.h_small, (const char*)P.keys[alt] + (size_t)(cnt - 1) * P.kb(), P.kb(), hipMemcpyDeviceToHost, P.stream));
            HIPCHK(hipStreamSynchronize(P.stream));
            dv.last_key = P.wide ? P.h_small[0] : (int64_t) * reinterpret_cast<const int32_t*>(P.h_small);
        }
    }
    return dv;
}

// K-pack of up to VIEW_SMALL_SLOTS slots by ONE launch, the count handed back through the pinned landing area of `P` (no tile counts, no scan, no
// copy, no stream synchronisation: 50 -> 15 us); returns -1 when the range does not qualify
int64_t pack_small(Pma& P, KeyArr k, const double* v, const uint64_t* occ, int64_t from, int64_t to, KeyArr ok, double* ov, int64_t out_cap) {
    if (to < from || from < 1 || to - from + 1 > VIEW_SMALL_SLOTS || to - from + 1 > out_cap) return -1;
    ViewAreaLease lease(P);
    const unsigned long long seq = ++P.view_seq;
    const SlotView raw{k, v, occ, to, nullptr, nullptr, nullptr, 0, true};      // a bare slot range: no tables, nothing is looked up
    LAUNCH("pack", launch_view_small(raw, 0, ok, ov, out_cap, P.d_small, P.h_view, 0, seq, from, to, P.stream));
    wait_handover(P, P.h_view + 5, seq, "pack");
    return P.h_view[4];
}

}  // namespace host
}  // namespace dsa
