// csrc/appendrun.hip — the per-op replay of an append run on the occupancy bitmap for gfx950.
//
// A run of setindex! calls with strictly ascending keys above the current last key (Coluna's column streaming, BASELINE
// config 2 batch A) always inserts behind the last cell, and the density scan / even rebalance that follows only needs
// cell COUNTS and produces cell POSITIONS — the keys and values never influence control flow.  Cells keep their relative
// order, so the final layout is a function of the final bitmap alone.  The run is therefore executed on the bitmap:
// wave 0 keeps the 4096-slot block around the tail in registers (one 64-bit word per lane, per-level counts as butterfly
// partial sums) and replays insert + _look_for_rebalance! + spread! per op without touching memory; windows wider than the
// block go through the workgroup-wide bitmap path.  The host then moves every cell exactly once (k_permute, rebalance.hip).
//     wave_model2_t          the tail inside the LAST occupancy word: scalar bit operations, memoised epochs ("model v2")
//     wave_fast_appends      the 4096-slot block around the tail in the registers of wave 0; calls the model where it applies
//     wave_apply_inblock     what the model left to write inside the last block
//     blk_rewrite_bits       spread! of a window wider than the block, bits only (workgroup)
//     blk_slow_append        one op on the global bitmap: any window, or the end of the run (_extend! / _shrink!)
//     k_run_expand           MappedPackedCSC: the ops of a run as a cell stream with one type bit per cell (semaphores)
//     k_append_run           the run: one workgroup, its own kernel so that the per-op loop of wave 0 stays spill-free
// The replay reads and writes occupancy words and counters only — its whole state is a SeqBits (seq_dev.h); keys, values,
// semaphores and the column tables are never touched here.  The sequencer detects a run and yields (sequencer.hip), the host
// launches the count-only models (appendmodel.hip) in front of k_append_run, which takes whatever they did not consume.
#include "seq_dev.h"

namespace dsa {

constexpr int64_t RUN_BLOCK = 4096;
constexpr int RUN_BLOCK_LOG2 = 12;

struct RunComm { int64_t idx, L, reb, slots, small; int32_t need, pad; };      // (spread_word_bits, spread_last_cell: dsa_dev.h)

// ---- model v2 of the append replay --------------------------------------------------------------------
// While the tail and the nearest gap stay inside the LAST occupancy word, an append is a handful of scalar bit operations on
// that word — set the bit behind the tail, or the nearest zero bit left of the last slot (the shift-left of _insert!,
// src/writes.jl:26-43) — and the density scan of the levels whose window fits the word (src/pma.jl:105-141) is a popcount
// of an aligned sub-mask per level; their spread! is a memoised bit pattern.  Levels wider than a word are suffixes of
// the array there: lane <-> level keeps their cell counts (+1 per append), a rebalance of level h with c cells resets the
// counts below it in closed form and yields the new last word.  The bitmap itself is written by the caller when the model
// is left: the last rebalance of every wide level that no wider one followed, widest first, then the last word.
// A separate, never inlined function with an LDS mailbox: every loop-carried value is re-established as wave-uniform
// (readfirstlane) so the loop compiles to scalar code with its own register allocation — inside the caller the same loop
// was placed in vector registers under exec masks and ran at 700 ns per op instead of ~100.
struct Model2IO {
    uint64_t lw; int64_t idx, end, reb, slots; int32_t need, progressed, nlow, seg;
    int32_t dbg_mid, dbg_miss, dbg_why, dbg_pad;      // dev counters (DSA_DBG_RUN)
    int64_t dbg_t[4];
    uint32_t cnt[64], W[64], Wb[64], lo[64], hi[64], ev_c[64], ev_valid[64];
    int32_t wb[64];
    uint32_t outside[64];        // level h wider than the block: cells of its suffix IN FRONT of the last block (workgroup pass)
    int32_t outside_valid;       // ... computed for the current bitmap
    int32_t pending;             // exit with rebalances wider than the block still to be written (workgroup), then the in-block ones
};
#ifdef DSA_M2_PROF
#define M2_T() clock64()
#else
#define M2_T() 0ll
#endif
struct RunMemo;
template <int NLOW, bool TYPED> __device__ __noinline__ void wave_model2_t(Model2IO* io, RunMemo* memo, const uint64_t* flags);

// words[]: memo of spread! patterns for windows of up to 256 slots: the pattern depends on (W, c) only and an append run keeps
// hitting the same few (level, count) pairs.  Filled on first use by wave 0.
constexpr int MEMO_ENTRIES = 640, MEMO_WORDS = 1664;
// memo entries: [0, M2_DIRECT) indexed by (level, count) for windows up to 256 slots, the rest hashed by (level, count).  The memo
// lives in dynamic LDS (128 KB of the CU's 160 KB: the kernel is one workgroup)
constexpr int M2_DIRECT = 512, M2_HASHED_LOG2 = 10, M2_HASHED = 1 << M2_HASHED_LOG2, M2_EV = M2_DIRECT + M2_HASHED;
constexpr int M2_HASH_LOG2 = 11, M2_HASH = 1 << M2_HASH_LOG2;
struct RunMemo {
    uint64_t words[MEMO_WORDS]; unsigned long long gapw[64];
    // model v2: memo of the rebalances of the wide levels, tagged (level << 16 | cell count) — windows up to 256 slots have their own
    // entry (level base + count), wider ones (up to the 4096-slot block) share a direct-mapped hash: counts of the wide levels below
    // (12 bits each), the last word after the rebalance, and the EPOCH that follows it — last word, number of in-word ops, their
    // rebalances and window slots — up to the next op that needs a wide level.  Epoch word: [7:0] ops + 1 (0: none) [8] partial
    // [16:9] rebalances [30:17] window slots [63:32] tag of the entry (0xffffffff: empty).
    struct alignas(16) M2Entry { uint64_t cnt, lw, eplw, epr; } m2e[M2_EV];      // one 32-byte entry: two 16-byte LDS loads, one wait
    // epochs keyed by the last word after the rebalance and the position of the first semaphore among the ops that follow (8: none
    // among the first eight): what the entry above cannot hold — rebalances of levels without an entry, and, in a typed run, epochs
    // that run through semaphore cells (`pat`: the cell types of the epoch's ops, bit k = op k is a semaphore).  Direct-mapped.
    struct alignas(16) M2Hash { uint64_t key, eplw, epr, pat; } m2h[M2_HASH];
    Model2IO m2;             // model v2: mailbox between wave_fast_appends and wave_model2
};   // gapw: scratch of the cooperative spread

__device__ __forceinline__ int ep_n(uint64_t r) { return (int)(r & 0xffu) - 1; }
__device__ __forceinline__ int ep_reb(uint64_t r) { return (int)((r >> 9) & 0xffu); }
__device__ __forceinline__ int ep_slots(uint64_t r) { return (int)((r >> 17) & 0x3fffu); }

// NLOW = number of levels whose window fits one occupancy word, a template parameter: the segment size (64 >> (NLOW - 1)), the
// level masks and the trip count of the in-word scan are constants of each instantiation, and the levels that do not exist cost no
// scalar registers (with six run-time levels the thresholds lived in spilled SGPRs, read back with v_readlane at every use).
// TYPED = the run has cell types (MappedPackedCSC: some cells are semaphores); a vector run carries none of that code.
template <int NLOW, bool TYPED> __device__ __noinline__ void wave_model2_t(Model2IO* io_, RunMemo* memo_, const uint64_t* flags_) {
    constexpr uint64_t TOP = 1ull << 63;
    // arguments of a non-kernel function arrive in vector registers and count as divergent: re-establish them as uniform
    Model2IO* io = (Model2IO*)readfirstlane64((uint64_t)io_);
    RunMemo* memo = (RunMemo*)readfirstlane64((uint64_t)memo_);
    const int lane = lane_id();
    uint64_t lw = readfirstlane64(io->lw);
    // ops are counted in 32 bits from a 64-aligned base (64-bit compares have no scalar form): op j is bit (j & 63) of cell-type word
    // fwp[j >> 6]; a longer run leaves at jend and comes back
    const int64_t idx0 = (int64_t)readfirstlane64((uint64_t)io->idx), end0 = (int64_t)readfirstlane64((uint64_t)io->end);
    const int64_t base = idx0 & ~63ll;
    const uint64_t* flags = (const uint64_t*)readfirstlane64((uint64_t)flags_);
    const uint64_t* fwp = TYPED ? flags + (base >> 6) : nullptr;
    constexpr bool typed = TYPED;                    // MappedPackedCSC run: some cells are semaphores
    int j = readfirstlane32((int)(idx0 - base));
    const int jend = readfirstlane32((int)(end0 - base < 0x7fff0000ll ? end0 - base : 0x7fff0000ll));
    constexpr int nlow = NLOW, seg = 64 >> (NLOW - 1);
    int lo_s[NLOW], hi_s[NLOW], wb_s[NLOW];
#pragma unroll
    for (int h = 0; h < NLOW; ++h) { lo_s[h] = readfirstlane32((int)io->lo[h]); hi_s[h] = readfirstlane32((int)io->hi[h]); wb_s[h] = readfirstlane32(io->wb[h]); }
    uint32_t cnt = io->cnt[lane];
    const uint32_t my_W = io->W[lane], my_lo = io->lo[lane], my_hi = io->hi[lane];
    const bool lvl_mid = my_W != 0;
    // memo of the wide levels: lane h holds the first entry of level h for windows up to 256 slots (entry = base + cell count);
    // wider levels hash (level, count) into [M2_DIRECT, M2_EV)
    int my_eb = -1;
    {
        int eb = 0;
        for (int h = nlow; h < 64; ++h) {
            const int Wh = seg << h;
            if (Wh > 256 || eb + Wh + 1 > M2_DIRECT) break;
            if (h == lane) my_eb = eb;
            eb += Wh + 1;
        }
    }
    auto entry_of = [&](int h, int c, int eb) -> int {
        // (levels whose lower wide levels would not fit the 5 x 12-bit counts of an entry — windows of more than 4096 slots — have none)
        return eb >= 0 ? eb + c : (h - nlow <= 5 ? M2_DIRECT + (int)((((uint32_t)h * 0x9E3779B1u) ^ ((uint32_t)c * 0x85EBCA6Bu)) >> (32 - M2_HASHED_LOG2)) : -1);
    };
    auto hslot_of = [&](uint64_t w, int p) -> int { return (int)(((w + (uint64_t)p) * 0x9E3779B97F4A7C15ull) >> (64 - M2_HASH_LOG2)); };
    const int my_k = lane - nlow < 0 ? 0 : (lane - nlow > 4 ? 4 : lane - nlow);
    const int my_sh = 12 * my_k;                     // where this level's count sits in a memo entry (at most 5 wide levels below the widest)
    uint32_t ev_c = 0;
    bool ev_valid = false;
    int reb = 0;
    int64_t slots = 0;
    int need = 0, progressed = 0, dbg_mid = 0, dbg_miss = 0, dbg_why = 0, dbg_jump = 0, dbg_ncmp = 0, dbg_sim = 0;
    int64_t dbg_tcmp = 0;
    [[maybe_unused]] int64_t pt_fast = 0, pt_sim = 0, pt_gen = 0;      // dev profile, -DDSA_M2_PROF
    [[maybe_unused]] int pn_fast = 0;
    const int64_t dbg_t0 = clock64();
    int fw_j = -1;                                   // cell-type word held in fw (index j >> 6)
    uint64_t fw = 0;
    // epoch being recorded: the in-word ops behind the rebalance that left the last word ep_key, up to the next op that needs a wide
    // level.  Cells only: it goes to the rebalance's memo entry (ep_entry >= 0) or, without one, to the hash under (ep_key, 8).  In a
    // typed run the cells in front of the first semaphore are recorded there as a PARTIAL epoch (it says nothing about the op behind
    // it), and the whole epoch with its cell types (at most 8 ops) goes to the hash under (ep_key, position of that semaphore).
    bool ep_on = false, ep_sem = false;
    int ep_entry = -1, ep_reb0 = 0, ep_j0 = 0;
    uint32_t ep_tag = 0, ep_pat = 0;
    uint64_t ep_key = 0;
    int64_t ep_slots0 = 0;
    bool wide_next = false;                          // the op at j is known to need a wide level (an epoch jump ended in front of it)
    auto pack_epoch = [&](bool partial, uint64_t hi32) -> uint64_t {      // 0: does not fit the fields
        const int n = j - ep_j0, nr = reb - ep_reb0;
        const int64_t ns = slots - ep_slots0;
        if (n > 254 || nr > 255 || ns > 16383) return 0ull;
        return (hi32 << 32) | ((uint64_t)ns << 17) | ((uint64_t)nr << 9) | (partial ? 0x100ull : 0ull) | (uint64_t)(n + 1);
    };
    auto record_plain = [&](bool partial) {          // cells only, up to (not including) op j
        const uint64_t r = pack_epoch(partial, ep_entry >= 0 ? (uint64_t)ep_tag : 0ull);
        if (r == 0 || lane != 0) return;
        if (ep_entry >= 0) { memo->m2e[ep_entry].eplw = lw; memo->m2e[ep_entry].epr = r; }
        else { RunMemo::M2Hash& hs = memo->m2h[hslot_of(ep_key, 8)]; hs.key = ep_key; hs.eplw = lw; hs.epr = r & 0xffffffffull; hs.pat = 0ull; }
    };
    auto start_epoch = [&](int entry, uint32_t tag, uint64_t key) {
        ep_on = true; ep_sem = false; ep_entry = entry; ep_tag = tag; ep_key = key; ep_pat = 0u; ep_j0 = j; ep_reb0 = reb; ep_slots0 = slots;
    };
    while (j < jend) {
        // (re-established as wave-uniform every iteration: the loop then stays on the scalar unit)
        lw = readfirstlane64(lw); j = readfirstlane32(j); reb = readfirstlane32(reb);
        const int64_t pt0 = M2_T();
        if (wide_next) {
            // ---- the common chain: an op that needs a wide level with a memo entry, followed by the recorded epoch of that entry.
            //      Straight-line and decided before anything is modified; every other case takes the general code below.
            const uint32_t cnt2 = cnt + (cnt < my_W ? 1u : 0u);
            const uint64_t acc = __ballot(lvl_mid && my_lo <= cnt2 && cnt2 <= my_hi);
            if (acc != 0) {
                const int h = __ffsll((unsigned long long)acc) - 1;
                const int c = (int)readlane32(cnt2, h);
                const int eb = (int)readlane32((uint32_t)my_eb, h);
                const int entry = entry_of(h, c, eb);
                if (entry >= 0) {
                    const RunMemo::M2Entry en = memo->m2e[entry];
                    const uint64_t r = readfirstlane64(en.epr);
                    const int n = ep_n(r);
                    bool ok = (uint32_t)(r >> 32) == (((uint32_t)h << 16) | (uint32_t)c) && n >= 0 && j + 1 + n < jend;
                    bool next_wide = (r & 0x100u) == 0;
                    if (typed && ok) {
                        // the n ops behind the event must be cells (one word of the type flags), and the op behind them too if it is to
                        // skip the in-word path
                        const int j1 = j + 1;
                        if ((j1 >> 6) != fw_j) { fw_j = j1 >> 6; fw = readfirstlane64(fwp[fw_j]); }
                        ok = ((j1 + n) >> 6) == fw_j;                              // (then n <= 63)
                        const uint64_t cells = ((1ull << (n & 63)) - 1ull) << (j1 & 63);
                        ok = ok && (fw & cells) == 0;
                        next_wide = next_wide && ((fw >> ((j1 + n) & 63)) & 1ull) == 0;
                    }
                    if (ok) {
                        const uint32_t below = (uint32_t)(en.cnt >> my_sh) & 0xfffu;
                        cnt = (lane < h && lvl_mid) ? below : cnt2;
                        if (lane == h) { ev_c = (uint32_t)c; ev_valid = true; }
                        else if (lane < h) ev_valid = false;
                        const uint32_t room = my_W - cnt;                  // cnt <= my_W
                        cnt += (uint32_t)n < room ? (uint32_t)n : room;
                        j += 1; reb += 1; slots += (int64_t)(seg << h);
                        if (r & 0x100u) {
                            // a partial epoch (it was cut by a semaphore when it was recorded): keep recording from the event on, a
                            // longer one replaces it when this visit gets further
                            start_epoch(entry, (uint32_t)(r >> 32), readfirstlane64(en.lw));
                        }
                        lw = readfirstlane64(en.eplw);
                        j += n; reb += ep_reb(r); slots += (int64_t)ep_slots(r);
                        progressed = 1; ++dbg_mid; ++dbg_jump;
                        wide_next = next_wide;
                        pt_fast += M2_T() - pt0; ++pn_fast;
                        continue;
                    }
                }
            }
        }
        bool is_sem = false;
        if (!wide_next) {
            if (typed) {
                if ((j >> 6) != fw_j) { fw_j = j >> 6; fw = readfirstlane64(fwp[fw_j]); }
                is_sem = (fw >> (j & 63)) & 1ull;
                if (is_sem && ep_on) {
                    if (!ep_sem) record_plain(true);              // the cells so far are a valid (partial) epoch of the entry
                    ep_sem = true;
                    if (j - ep_j0 < 8) ep_pat |= 1u << (j - ep_j0); else ep_on = false;
                }
            }
            // ---- the insert, on the last word  (a branch-free form of this block — selects between the three inserts, all six
            //      levels evaluated — was measured slower: 12.6 vs 10.2 ms per 41 k appends; the cost is instructions, not branches)
            uint64_t nw = lw;
            int bip;                                   // bit of the insert position
            if (lw & TOP) {                            // tail on the last slot: the cells behind the nearest gap shift left
                const uint64_t z = ~lw;
                if (z == 0) { dbg_why = 1; break; }    // that gap is in an earlier word: general path
                nw |= 1ull << (63 - __clzll((long long)z));
                bip = 63;
            } else if (!is_sem) {                      // behind the tail
                if (lw == 0) { dbg_why = 2; break; }
                bip = 64 - __clzll((long long)lw);
                nw |= 1ull << bip;
            } else {                                   // a semaphore goes to the last slot (src/pcsr.jl:99-112)
                const uint64_t z = ~lw & ~TOP;
                if (z == 0) { dbg_why = 1; break; }
                const int pe = 63 - __clzll((long long)z);
                if (pe == 62) nw |= TOP;
                else nw = (nw | (1ull << pe) | TOP) & ~(1ull << 62);
                bip = 63;
            }
            // ---- _look_for_rebalance!, levels inside the word
            int h_acc = -1, c_acc = 0, sh_acc = 0, wbh = 0;
#pragma unroll
            for (int h = 0; h < NLOW; ++h) {
                const int W = seg << h;
                const int sh = bip & ~(W - 1);
                const uint64_t m = (W == 64 ? ~0ull : ((1ull << W) - 1ull)) << sh;
                const int c = popc64(nw & m);
                if (lo_s[h] <= c && c <= hi_s[h]) { h_acc = h; c_acc = c; sh_acc = sh; wbh = wb_s[h]; break; }
            }
            if (h_acc >= 0) {
                if (h_acc > 0) {                       // _even_rebalance! inside the word: memoised pattern of (W, c)
                    const int W = seg << h_acc;
                    uint64_t pat = readfirstlane64(memo->words[wbh + c_acc]);
                    if (pat == 0) {
                        ++dbg_miss;
                        SpreadGeom g;
                        g.W = W; g.E = W - c_acc;
                        g.f = (double)W / (double)(W - c_acc);
                        g.inv_f = (double)(W - c_acc) / (double)W;
                        int rank;
                        const bool cell = lane < W && !slot_is_gap(g, lane + 1, &rank);
                        pat = __ballot(cell);
                        if (lane == 0) memo->words[wbh + c_acc] = pat;
                    }
                    const uint64_t m = (W == 64 ? ~0ull : ((1ull << W) - 1ull)) << sh_acc;
                    nw = (nw & ~m) | (pat << sh_acc);
                    reb += 1; slots += W;
                }
                lw = nw;
                cnt += cnt < my_W ? 1u : 0u;
                ++j; progressed = 1; ++dbg_sim;
                pt_sim += M2_T() - pt0;
                continue;
            }
        }
        wide_next = false;
        // ---- the op needs a level wider than a word.  The epoch being recorded ends in front of it.
        if (ep_on) {
            if (!ep_sem) record_plain(false);
            else if (j - ep_j0 < 8) {
                // the whole epoch with its cell types, under (last word behind the rebalance, position of the first semaphore)
                const uint32_t pat = ep_pat | (is_sem ? 1u << (j - ep_j0) : 0u);          // bit n: the op that did not fit
                const uint64_t r = pack_epoch(false, 0ull);
                if (r != 0 && lane == 0) {
                    RunMemo::M2Hash& hs = memo->m2h[hslot_of(ep_key, __ffs((int)ep_pat) - 1)];
                    hs.key = ep_key; hs.eplw = lw; hs.epr = r; hs.pat = (uint64_t)pat;
                }
            }
            ep_on = false;
        }
        const uint32_t cnt2 = cnt + (cnt < my_W ? 1u : 0u);
        const uint64_t acc = __ballot(lvl_mid && my_lo <= cnt2 && cnt2 <= my_hi);
        if (acc == 0) { need = 1; dbg_why = 3; break; }         // a window wider than the block (or _extend!) decides
        cnt = cnt2;
        ++j; progressed = 1; ++dbg_mid;
        const int h = __ffsll((unsigned long long)acc) - 1;
        const int W = seg << h;
        const int c = (int)readlane32(cnt, h);
        reb += 1; slots += W;
        if (lane == h) { ev_c = (uint32_t)c; ev_valid = true; }
        else if (lane < h) ev_valid = false;
        const int eb = (int)readlane32((uint32_t)my_eb, h);
        const int entry = entry_of(h, c, eb);
        const uint32_t tagv = ((uint32_t)h << 16) | (uint32_t)c;
        uint64_t e = 0, en_lw = 0, en_eplw = 0, en_epr = 0;
        bool filled = false;
        if (entry >= 0) {
            const RunMemo::M2Entry en = memo->m2e[entry];
            e = readfirstlane64(en.cnt); en_lw = readfirstlane64(en.lw); en_eplw = readfirstlane64(en.eplw); en_epr = readfirstlane64(en.epr);
            filled = (uint32_t)(en_epr >> 32) == tagv;
        }
        if (!filled) {
            en_epr = 0;
            const int64_t tc0 = clock64();
            ++dbg_ncmp;
            SpreadGeom g;
            g.W = W; g.E = W - c;
            g.f = (double)W / (double)(W - c);
            g.inv_f = (double)(W - c) / (double)W;
            uint32_t below = 0;
            if (lane < h && lvl_mid) below = my_W - (uint32_t)((W - c) - gaps_le(g, W - (int)my_W));
            int rank;
            const bool cell = !slot_is_gap(g, W - 63 + lane, &rank);
            lw = __ballot(cell);
            if (lane < h && lvl_mid) cnt = below;
            if (entry >= 0) {          // counts of the (at most five) wide levels below h, 12 bits each (a level below h holds < 4096 slots)
                e = (uint64_t)readlane32(below, nlow) | ((uint64_t)readlane32(below, nlow + 1) << 12) | ((uint64_t)readlane32(below, nlow + 2) << 24) |
                    ((uint64_t)readlane32(below, nlow + 3) << 36) | ((uint64_t)readlane32(below, nlow + 4) << 48);
                if (lane == 0) { memo->m2e[entry].cnt = e; memo->m2e[entry].lw = lw; memo->m2e[entry].epr = (uint64_t)tagv << 32; }
            }
            dbg_tcmp += clock64() - tc0;
        } else {
            if (lane < h && lvl_mid) cnt = (uint32_t)(e >> my_sh) & 0xfffu;
            lw = en_lw;
        }
        // ---- the in-word ops that follow are a function of the new last word and of their cell types alone: replay them from the memo
        uint32_t pat8 = 0;                             // cell types of the next (up to 8) ops, as far as the current type word reaches
        int pat_n = 8;
        if (typed) {
            if ((j >> 6) != fw_j) { fw_j = j >> 6; fw = readfirstlane64(fwp[fw_j]); }
            pat8 = (uint32_t)(fw >> (j & 63)) & 0xffu;
            pat_n = 64 - (j & 63) < 8 ? 64 - (j & 63) : 8;
            pat8 &= (1u << pat_n) - 1u;
        }
        const int p_sem = pat8 != 0 ? __ffs((int)pat8) - 1 : 8;      // position of the first semaphore among the next ops (8: none)
        // the hash: (last word, position of the first semaphore) — rebalances without an entry, and epochs that run through semaphores
        auto try_hash = [&](int p) -> bool {
            const RunMemo::M2Hash hs = memo->m2h[hslot_of(lw, p)];
            const uint64_t r = readfirstlane64(hs.epr);
            const int n = ep_n(r);
            const uint32_t hp = (uint32_t)readfirstlane64(hs.pat);
            bool ok = readfirstlane64(hs.key) == lw && n >= 0 && j + n < jend;
            if (ok && typed) {
                if (p < 8) ok = n + 1 <= pat_n && ((pat8 ^ hp) & ((2u << n) - 1u)) == 0;          // the same types for the n ops and the op behind them
                else ok = hp == 0 && (j >> 6) == ((j + n) >> 6) && (fw & (((2ull << (n & 63)) - 1ull) << (j & 63))) == 0;
            }
            if (!ok) return false;
            lw = readfirstlane64(hs.eplw);
            j += n;
            const uint32_t room = my_W - cnt;                      // cnt <= my_W
            cnt += (uint32_t)n < room ? (uint32_t)n : room;
            reb += ep_reb(r); slots += (int64_t)ep_slots(r);
            // the op behind it had this type when the epoch was recorded and needed a wide level: it does again (kept to cells)
            wide_next = (r & 0x100u) == 0 && !((hp >> n) & 1u);      // (a partial epoch says nothing about the op behind it)
            ++dbg_jump;
            if (p == 8 && entry >= 0 && lane == 0) { memo->m2e[entry].eplw = lw; memo->m2e[entry].epr = ((uint64_t)tagv << 32) | (r & 0xffffffffull); }
            return true;
        };
        bool jumped = false;
        if (p_sem < 8) jumped = try_hash(p_sem);
        if (!jumped) {
            // the cells-only epoch of the entry
            const uint64_t r = en_epr;
            const int n = ep_n(r);
            bool cells_only = true;
            if (typed && n > 0) {
                if ((j >> 6) != ((j + n - 1) >> 6)) cells_only = false;
                else cells_only = (fw & (((1ull << (n & 63)) - 1ull) << (j & 63))) == 0;
            }
            if (n >= 0 && j + n < jend && cells_only) {
                if (r & 0x100u) start_epoch(entry, tagv, lw);      // partial epoch: go on recording, a longer one replaces it
                lw = en_eplw;
                j += n;
                const uint32_t room = my_W - cnt;                  // cnt <= my_W
                cnt += (uint32_t)n < room ? (uint32_t)n : room;
                reb += ep_reb(r); slots += (int64_t)ep_slots(r);
                // the op behind a complete epoch was a cell when it was recorded (it did not fit the word): the same holds now if it is a
                // cell again; a semaphore there may still fit the word and takes the in-word path first.  A partial epoch says nothing.
                wide_next = (r & 0x100u) == 0 && (!typed || ((j >> 6) == fw_j && ((fw >> (j & 63)) & 1ull) == 0));
                ++dbg_jump;
                jumped = true;
            }
        }
        if (!jumped && p_sem == 8) jumped = try_hash(8);
        if (!jumped) start_epoch(entry, tagv, lw);
        pt_gen += M2_T() - pt0;
    }
    io->ev_c[lane] = ev_c; io->ev_valid[lane] = ev_valid ? 1u : 0u;
    if (lane == 0) { io->lw = lw; io->idx = base + j; io->need = need; io->progressed = progressed; io->reb = reb; io->slots = slots;
                     io->dbg_mid = dbg_mid; io->dbg_miss = dbg_miss; io->dbg_why = dbg_why; io->dbg_pad = dbg_sim; io->dbg_t[0] = dbg_jump; io->dbg_t[1] = dbg_ncmp; io->dbg_t[2] = dbg_tcmp; io->dbg_t[3] = clock64() - dbg_t0;
#ifdef DSA_M2_PROF
                     printf("m2 prof: fast %d events %lld clk, sim %d ops %lld clk, general %d events %lld clk, total %lld\n", pn_fast, (long long)pt_fast, dbg_sim, (long long)pt_sim, dbg_mid - pn_fast, (long long)pt_gen, (long long)(clock64() - dbg_t0));
#endif
    }
}

// wave 0: replays appends rc->idx .. end-1 on the register-resident block until one needs the workgroup path (need = 1).
// Everything per op is wave-uniform register work: lane <-> occupancy word of the block for the bitmap, lane <-> level
// for the density scan (the levels inside one word are tested first, from the word alone; wider in-block levels from a
// butterfly of word popcounts), lane <-> window offset when a spread! pattern is computed (one ballot per word).
// spread! of c cells over the W-slot window starting at slot ws, bits only, on the register-resident block (lane <-> occupancy
// word; lw0 = lane of the window's first word; wb_level = memo base of the level, used when W <= 256).  Returns the position of
// the window's last cell.
template <typename P>
__device__ __forceinline__ P wave_spread_bits(uint64_t& word, RunMemo* memo, int lane, int W, int c, int wb_level, P ws, int lw0) {
    if (W <= 256) {
        const int nw = W < 64 ? 1 : (W >> 6);
        const int wb = wb_level + c * nw;
        // a filled entry never ends with an empty word (c >= lo[h] cells spread evenly): 0 = not computed yet — one LDS
        // round trip instead of a separate valid flag
        uint64_t lastw = memo->words[wb + nw - 1];
        if (lastw == 0) {
            SpreadGeom g;                                             // make_geom(W, c) with 32-bit conversions
            g.W = W; g.E = W - c;
            g.f = (double)W / (double)(W - c);
            g.inv_f = (double)(W - c) / (double)W;
            for (int t = 0; t < nw; ++t) {
                const int q = 64 * t + lane + 1;
                int rank;
                const bool cell = q <= W && !slot_is_gap(g, q, &rank);
                const uint64_t nb = __ballot(cell);
                if (lane == 0) memo->words[wb + t] = nb;
                lastw = nb;
            }
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_s_waitcnt(0xc07f);                        // the other lanes read the entry below
        }
        if (W < 64) {
            const int sh = (int)((ws - 1) & 63);
            const uint64_t m = ((1ull << W) - 1ull) << sh;
            if (lane == lw0) word = (word & ~m) | (lastw << sh);
        } else {
            const int t = lane - lw0;
            if (t >= 0 && t < nw) word = memo->words[wb + t];
        }
        return ws - 1 + 64 * (nw - 1) + (64 - __clzll((long long)lastw));
    }
    SpreadGeom g;
    g.W = W; g.E = W - c;
    g.f = (double)W / (double)(W - c);
    g.inv_f = (double)(W - c) / (double)W;
    const int t = lane - lw0;
    const int nww = W >> 6, E = W - c;
    if (E <= 16 * nww) {
        // few gaps per word (dense window): the whole wave generates the E gap offsets D(k) — lane <-> k — and clears
        // their bits in an LDS image of the window, instead of every lane looping over the gaps of its own word
        if (lane < nww) memo->gapw[lane] = ~0ull;
        __builtin_amdgcn_wave_barrier();
        for (int k = lane + 1; k <= E; k += 64) {
            const int d = gap_D(g, k);                             // 1-based offset in the window
            atomicAnd(&memo->gapw[(d - 1) >> 6], ~(1ull << ((d - 1) & 63)));
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_s_waitcnt(0xc07f);                        // lgkmcnt(0): the wave's LDS atomics have landed
        if (t >= 0 && t < nww) word = memo->gapw[t];
        __builtin_amdgcn_wave_barrier();
    } else if (t >= 0 && t < nww) word = spread_word_bits(g, t);
    return ws - 1 + (P)spread_last_cell(g);
}

// P = int32_t while capacity and run length fit 30 bits (positions, op indices and word indices are then single-register values:
// a lone wave issues ~1 instruction per 4 cycles, so halving the 64-bit arithmetic is what shortens an op), int64_t otherwise.
template <typename P>
__device__ void wave_fast_appends(SeqBits& S, RunComm* rc, RunMemo* memo, const uint64_t* flags, int64_t end64) {
    const P end = (P)end64;
    const int lane = lane_id();
    P idx = (P)rc->idx, L = (P)rc->L;
    int64_t reb = 0, slots = 0;
    const P cap = (P)S.capacity, seg = (P)S.seg;
    const int height = (int)S.height;
    const P nwords = (cap + 63) >> 6;
    const P blkslots = cap < (P)RUN_BLOCK ? cap : (P)RUN_BLOCK;
    const int lseg = 63 - __clzll((long long)seg);
    // level h = lane: window size and integer density bounds; levels wider than the block cannot be decided here
    const bool lvl_valid = lane <= height;
    const int64_t Wl = lvl_valid ? ((int64_t)seg << lane) : 0;
    const bool lvl_in_block = lvl_valid && Wl <= blkslots;
    const bool lvl_low = lvl_in_block && Wl <= 64;
    const bool lvl_mid = lvl_in_block && Wl > 64;
    const uint32_t my_lo = lvl_in_block ? (uint32_t)S.lo[lane] : 1u;
    const uint32_t my_hi = lvl_in_block ? (uint32_t)S.hi[lane] : 0u;
    const int my_j = lvl_mid ? (lseg + lane - 6) : 0;                           // log2(W / 64)
    const uint64_t my_low_mask = lvl_low ? (Wl == 64 ? ~0ull : ((1ull << Wl) - 1ull)) : 0ull;
    const int my_low_align = lvl_low ? ~((int)Wl - 1) & 63 : 0;
    const bool any_mid = __ballot(lvl_mid) != 0;
    // memo base of level h = lane (W <= 256): first word of entry c = 0
    int my_wb = 0;
    {
        int wb = 0;
        for (int h = 0; h < 64; ++h) {
            const int64_t Wh = (int64_t)seg << h;
            if (h > height || Wh > 256) break;
            if (h == lane) my_wb = wb;
            wb += ((int)Wh + 1) * (Wh <= 64 ? 1 : (int)(Wh >> 6));
        }
    }
    const int last_lane = (int)((nwords - 1) & 63);
    const uint64_t cap_bit = 1ull << ((cap - 1) & 63);
    int need = 0;
    // model v2: the last word is simulated bit-exactly, wider levels by their suffix counts (whole 4096-slot block in front of the end: last_lane == 63)
    const int nlow = 7 - lseg;                                      // levels whose window fits one occupancy word (W = seg << h <= 64)
    const bool model2_ok = cap >= (P)RUN_BLOCK && rc->pad == 0 && nlow >= 1 && nlow <= 6 && (int)seg << (nlow - 1) == 64;
    bool skip_model = false;                                        // the model could not place the current op: one op through the general path
    bool wrote_block = true;                                        // false: the block in registers is discarded (the workgroup rewrites wider windows first)
    const P last_blk = (cap - 1) >> RUN_BLOCK_LOG2;
    // cell types of the run (MappedPackedCSC: bit set = semaphore cell of a new column); one word per 64 cells
    P fw_idx = -1;
    uint64_t fw = 0;
    while (idx < end && need == 0) {
        if (flags != nullptr && (idx >> 6) != fw_idx) { fw_idx = idx >> 6; fw = flags[fw_idx]; }
        const bool sem0 = (fw >> (idx & 63)) & 1ull;
        const P tgt = (L < cap && !sem0) ? L + 1 : cap;
        const P blk = (tgt - 1) >> RUN_BLOCK_LOG2;
        const P w = blk * 64 + lane;
        uint64_t word = w < nwords ? S.occ[w] : 0ull;
        while (idx < end) {
            if (flags != nullptr && (idx >> 6) != fw_idx) { fw_idx = idx >> 6; fw = flags[fw_idx]; }
            const bool is_sem = (fw >> (idx & 63)) & 1ull;
            // ---- count model: the tail sits on the last slot of the array.  Every append — cell or semaphore —
            //      then takes the nearest gap left of the last slot and the windows of the density scan are the SUFFIXES of the array,
            //      so the replay only needs the suffix count of every level (lane <-> level): an append adds 1 to every level
            //      whose suffix still has a gap; a rebalance of level h with c cells leaves level j < h with W_j - G_j cells, G_j =
            //      gaps of the closed-form spread pattern that fall into the last W_j offsets.  The bitmap is not touched per op:
            //      when the model is left, the LAST rebalance of every level (each still valid outside the suffix of the next lower
            //      one) is written once and the gaps consumed since — all in the last leaf — are filled from the right.
            // ---- model v2 (wave_model2 below): the last occupancy word simulated bit-exactly, wider levels by suffix counts
            if (model2_ok && !skip_model && blk == last_blk && L > cap - 64 && !memo->m2.outside_valid) { need = 3; break; }   // the workgroup recounts first
            if (model2_ok && !skip_model && blk == last_blk && L > cap - 64) {
                Model2IO* io = &memo->m2;
                {
                    uint32_t sb[7];
                    sb[0] = (uint32_t)popc64(word);
#pragma unroll
                    for (int j = 1; j < 7; ++j) sb[j] = sb[j - 1] + __shfl_xor(sb[j - 1], 1 << (j - 1), 64);
                    const uint32_t s1 = readlane32(sb[1], 63), s2 = readlane32(sb[2], 63), s3 = readlane32(sb[3], 63), s4 = readlane32(sb[4], 63),
                                   s5 = readlane32(sb[5], 63), s6 = readlane32(sb[6], 63);
                    const uint32_t c_mid = my_j == 1 ? s1 : my_j == 2 ? s2 : my_j == 3 ? s3 : my_j == 4 ? s4 : my_j == 5 ? s5 : s6;
                    // levels wider than the block: cells in front of the block (io->outside, workgroup pass) + the whole block
                    io->cnt[lane] = lvl_mid ? c_mid : (lvl_valid && !lvl_in_block ? io->outside[lane] + s6 : 0u);
                }
                io->W[lane] = lvl_valid && Wl > 64 ? (uint32_t)Wl : 0u;
                io->Wb[lane] = lvl_in_block ? (uint32_t)Wl : 0u;
                io->lo[lane] = lvl_valid ? (uint32_t)S.lo[lane] : 1u; io->hi[lane] = lvl_valid ? (uint32_t)S.hi[lane] : 0u;
                io->wb[lane] = my_wb;
                if (lane == 0) {
                    io->lw = readlane64(word, 63); io->idx = (int64_t)idx; io->end = (int64_t)end; io->nlow = nlow; io->seg = (int)seg;
                    io->need = 0; io->progressed = 0; io->reb = 0; io->slots = 0;
                }
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_s_waitcnt(0xc07f);
                if (flags != nullptr) {
                    switch (nlow) {
                        case 1: wave_model2_t<1, true>(io, memo, flags); break;
                        case 2: wave_model2_t<2, true>(io, memo, flags); break;
                        case 3: wave_model2_t<3, true>(io, memo, flags); break;
                        case 4: wave_model2_t<4, true>(io, memo, flags); break;
                        case 5: wave_model2_t<5, true>(io, memo, flags); break;
                        default: wave_model2_t<6, true>(io, memo, flags); break;
                    }
                } else {
                    switch (nlow) {
                        case 1: wave_model2_t<1, false>(io, memo, flags); break;
                        case 2: wave_model2_t<2, false>(io, memo, flags); break;
                        case 3: wave_model2_t<3, false>(io, memo, flags); break;
                        case 4: wave_model2_t<4, false>(io, memo, flags); break;
                        case 5: wave_model2_t<5, false>(io, memo, flags); break;
                        default: wave_model2_t<6, false>(io, memo, flags); break;
                    }
                }
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_s_waitcnt(0xc07f);
                if (lane == 0) { S.ctl->prof[8] += 1; S.ctl->prof[9] += io->idx - (int64_t)idx; S.ctl->prof[10] += io->dbg_mid; S.ctl->prof[11] += io->dbg_miss;
                                 S.ctl->prof[12 + (io->dbg_why & 3)] += 1; S.ctl->prof[3] += io->dbg_pad; S.ctl->prof[4] += io->dbg_t[0]; S.ctl->prof[5] += io->dbg_t[1]; S.ctl->prof[6] += io->dbg_t[2]; S.ctl->prof[7] += io->dbg_t[3]; }
                idx = (P)io->idx; reb += io->reb; slots += io->slots;
                const uint64_t lw = io->lw;
                fw_idx = -1;                                   // (the callee read the cell-type words itself)
                if (lw != 0) L = cap - 63 + (P)(63 - __clzll((long long)lw));
                // the surviving wide rebalances, widest first, then the last word.  Windows wider than the block are written by the
                // whole workgroup (k_append_run), which then calls wave_apply_inblock for the rest
                const uint64_t vm_all = __ballot(io->ev_valid[lane] != 0);
                const uint64_t vm_out = vm_all & __ballot(lvl_valid && !lvl_in_block);
                if (vm_out != 0) {
                    if (lane == 0) io->pending = 1;
                    need = io->need ? 1 : 2;
                    wrote_block = false;
                    break;
                }
                uint64_t vm = vm_all;
                const uint32_t ev_c = io->ev_c[lane];
                while (vm != 0) {
                    const int j = 63 - __clzll((long long)vm);
                    vm &= ~(1ull << j);
                    const int Wj = (int)seg << j;
                    const P wsj = cap - Wj + 1;
                    wave_spread_bits<P>(word, memo, lane, Wj, (int)readlane32(ev_c, j), (int)readlane32((uint32_t)my_wb, j), wsj, (int)(((wsj - 1) >> 6) & 63));
                }
                if (lane == 63) word = lw;
                if (io->need) { need = 1; break; }
                skip_model = io->progressed == 0;
                continue;
            }
            skip_model = false;
            const uint64_t word_saved = word;
            P ip;
            if (L < cap && !is_sem) {
                // _insert! behind the last cell  src/writes.jl:26-43
                ip = L + 1;
                if (((ip - 1) >> RUN_BLOCK_LOG2) != blk) break;                       // the tail moves into the next block: reload
                if (lane == (int)(((ip - 1) >> 6) & 63)) word |= 1ull << ((ip - 1) & 63);
            } else {
                // insert at the end of the array: a cell behind a tail that sits on the last slot, or a new partition's
                // semaphore (always inserted "after position capacity", src/pcsr.jl:99-112).  The nearest empty slot left
                // of the last slot takes the shift; almost always it is in the last word.
                if (((cap - 1) >> RUN_BLOCK_LOG2) != blk) break;
                const uint64_t wl = readlane64(word, last_lane);
                uint64_t zl = ~wl & ~cap_bit;
                if (cap < 64) zl &= (1ull << cap) - 1ull;
                uint32_t best;
                if (zl) best = (uint32_t)((last_lane << 6) + 64 - __clzll((long long)zl));
                else {
                    uint64_t z = w < nwords ? ~word : 0ull;
                    if (lane == last_lane) z &= ~cap_bit;
                    const uint32_t rel = z ? (uint32_t)((lane << 6) + 64 - __clzll((long long)z)) : 0u;
                    best = wave_max_u32(rel);
                    if (best == 0) { need = 1; break; }
                }
                const P pe = blk * (P)RUN_BLOCK + (P)best;
                ip = cap;
                if (wl & cap_bit) {                                           // tail on the last slot: cells (pe, cap] shift left
                    if (lane == (int)(((pe - 1) >> 6) & 63)) word |= 1ull << ((pe - 1) & 63);
                } else if (pe == cap - 1) {                                   // last slot and its neighbour empty
                    if (lane == last_lane) word |= cap_bit;
                } else {                                                      // last slot empty, cells (pe, cap-1] shift left
                    if (lane == (int)(((pe - 1) >> 6) & 63)) word |= 1ull << ((pe - 1) & 63);
                    if (lane == (int)(((cap - 2) >> 6) & 63)) word &= ~(1ull << ((cap - 2) & 63));
                    if (lane == last_lane) word |= cap_bit;
                }
            }
            const int lane_ip = __builtin_amdgcn_readfirstlane((int)(((ip - 1) >> 6) & 63));
            const int bit_ip = (int)((ip - 1) & 63);
            // _look_for_rebalance!  src/pma.jl:105-141: lane h evaluates level h
            const uint64_t word_ip = readlane64(word, lane_ip);
            uint32_t c_l = (uint32_t)popc64(word_ip & (my_low_mask << (bit_ip & my_low_align)));
            uint64_t acc = __ballot(lvl_low && my_lo <= c_l && c_l <= my_hi);
            if (acc == 0 && any_mid) {
                uint32_t s[7];
                s[0] = (uint32_t)popc64(word);
#pragma unroll
                for (int j = 1; j < 7; ++j) s[j] = s[j - 1] + __shfl_xor(s[j - 1], 1 << (j - 1), 64);
                const uint32_t s1 = readlane32(s[1], lane_ip), s2 = readlane32(s[2], lane_ip), s3 = readlane32(s[3], lane_ip),
                               s4 = readlane32(s[4], lane_ip), s5 = readlane32(s[5], lane_ip), s6 = readlane32(s[6], lane_ip);
                c_l = my_j == 1 ? s1 : my_j == 2 ? s2 : my_j == 3 ? s3 : my_j == 4 ? s4 : my_j == 5 ? s5 : s6;
                acc = __ballot(lvl_mid && my_lo <= c_l && c_l <= my_hi);
            }
            if (acc == 0) {
                // a wider window (or _extend!) decides: undo, hand the op to the workgroup path
                word = word_saved;
                need = 1;
                break;
            }
            const int h = __ffsll((unsigned long long)acc) - 1;
            if (blk != last_blk && memo->m2.outside_valid) { if (lane == 0) memo->m2.outside_valid = 0; }     // cells in front of the last block changed
            if (h == 0) { L = ip; ++idx; continue; }
            // _even_rebalance!: spread! of c cells over the window, bits only
            const int W = (int)seg << h;                                      // <= 4096
            const int c = (int)readlane32(c_l, h);
            reb += 1; slots += W;
            const P ws = ((ip - 1) & ~((P)W - 1)) + 1;
            const int lw0 = (int)(((ws - 1) >> 6) & 63);
            L = wave_spread_bits<P>(word, memo, lane, W, c, (int)readlane32((uint32_t)my_wb, h), ws, lw0);
            ++idx;
        }
        if (w < nwords && wrote_block) S.occ[w] = word;
        wrote_block = true;
    }
    if (lane == 0) { rc->idx = (int64_t)idx; rc->L = (int64_t)L; rc->reb = reb; rc->slots = slots; rc->small = reb; rc->need = need; }
}

// model v2, second half of an exit that had rebalances wider than the block (written by the workgroup in between): the in-block
// survivors, widest first, then the last word, on the last block of the bitmap.  Wave 0.
__device__ void wave_apply_inblock(SeqBits& S, RunMemo* memo) {
    const int lane = lane_id();
    Model2IO* io = &memo->m2;
    const int64_t cap = S.capacity, seg = S.seg;
    const int height = (int)S.height;
    const int64_t last_blk = (cap - 1) >> RUN_BLOCK_LOG2;
    const int64_t w = last_blk * 64 + lane;
    uint64_t word = S.occ[w];
    int my_wb = 0;                      // memo base of level h = lane (W <= 256), as in wave_fast_appends
    {
        int wb = 0;
        for (int h = 0; h < 64; ++h) {
            const int64_t Wh = seg << h;
            if (h > height || Wh > 256) break;
            if (h == lane) my_wb = wb;
            wb += ((int)Wh + 1) * (Wh <= 64 ? 1 : (int)(Wh >> 6));
        }
    }
    const bool in_block = lane <= height && (seg << lane) <= RUN_BLOCK && (seg << lane) > 64;
    uint64_t vm = __ballot(in_block && io->ev_valid[lane] != 0);
    const uint32_t ev_c = io->ev_c[lane];
    while (vm != 0) {
        const int j = 63 - __clzll((long long)vm);
        vm &= ~(1ull << j);
        const int Wj = (int)(seg << j);
        const int64_t wsj = cap - Wj + 1;
        wave_spread_bits<int64_t>(word, memo, lane, Wj, (int)readlane32(ev_c, j), (int)readlane32((uint32_t)my_wb, j), wsj, (int)(((wsj - 1) >> 6) & 63));
    }
    if (lane == 63) word = io->lw;
    S.occ[w] = word;
}

// spread! of m cells over [ws, we], occupancy words only (workgroup-wide)
__device__ void blk_rewrite_bits(SeqBits& S, int64_t ws, int64_t we, int64_t m) {
    const int64_t W = we - ws + 1;
    const SpreadGeom g = make_geom(W, m);
    const int64_t w0 = (ws - 1) >> 6;
    __syncthreads();
    if (W >= 64) {
        for (int64_t t = threadIdx.x; t < (W >> 6); t += SEQ_BLOCK) S.occ[w0 + t] = spread_word_bits(g, (int)t);
    } else if (threadIdx.x == 0) {
        const int sh = (int)((ws - 1) & 63);
        const uint64_t msk = ((1ull << W) - 1ull) << sh;
        S.occ[w0] = (S.occ[w0] & ~msk) | ((spread_word_bits(g, 0) << sh) & msk);
    }
    __syncthreads();
}

// one append on the global bitmap (all threads, uniform): insert behind the tail (or, for a semaphore / a tail on the
// last slot, at the end of the array) + density scan + spread! of the bits.  Returns false (bitmap unchanged) when the op
// needs _extend! / _shrink! or cannot be placed: the run ends before it.
__device__ bool blk_slow_append(SeqBits& S, int64_t& L, bool is_sem) {
    const int64_t cap = S.capacity;
    int64_t ip, pe = 0;
    int how;                      // 0: set ip ; 1: set pe ; 2: set cap ; 3: set pe, clear cap-1, set cap
    if (L < cap && !is_sem) { ip = L + 1; how = 0; }
    else {
        pe = d_prev_empty(S.occ, cap);
        if (pe == 0) return false;
        ip = cap;
        how = occ_test(S.occ, cap) ? 1 : (pe == cap - 1 ? 2 : 3);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (how == 0) occ_set(S, ip);
        else if (how == 1) occ_set(S, pe);
        else if (how == 2) occ_set(S, cap);
        else { occ_set(S, pe); occ_clear(S, cap - 1); occ_set(S, cap); }
    }
    __syncthreads();
    int64_t prev_ws = ip, prev_we = ip - 1, left = 0, right = 0, ws = 1, we = cap;
    bool accepted = false;
    int64_t h0 = 0;
    if (cap >= 4096) {
        // Levels up to 65536 slots in ONE pass instead of two block-wide counts (four barriers) per level: every word of the
        // aligned 65536-slot window around ip adds its popcount to the bucket of the smallest whole-word window that holds both
        // it and ip's word; the count of a level is a prefix sum over the buckets (levels inside one word: masks of ip's word).
        __shared__ unsigned int sBk[12];
        const int64_t PW = cap < 65536 ? cap : 65536;
        const int64_t wsP = ((ip - 1) & ~(PW - 1)) + 1;
        const int64_t w0 = (wsP - 1) >> 6, nw = PW >> 6, ipw = (ip - 1) >> 6;
        if (threadIdx.x < 12) sBk[threadIdx.x] = 0u;
        __syncthreads();
        for (int64_t k = threadIdx.x; k < nw; k += SEQ_BLOCK) {
            const int64_t w = w0 + k;
            const uint64_t x = (uint64_t)(w ^ ipw);
            atomicAdd(&sBk[x ? 64 - __clzll((long long)x) : 0], (unsigned int)popc64(S.occ[w]));
        }
        __syncthreads();
        const uint64_t wip = S.occ[ipw];
        const int bip = (int)((ip - 1) & 63);
        int64_t c = 0, h = 0;
        for (; h <= S.height && (S.seg << h) <= PW; ++h) {
            const int64_t W = S.seg << h;
            if (W < 64) c = popc64(wip & ((((uint64_t)1 << W) - 1ull) << (bip & ~((int)W - 1))));
            else {
                const int lw = 63 - __clzll((long long)(W >> 6));          // window of 2^lw words
                c = 0;
                for (int k = 0; k <= lw; ++k) c += sBk[k];
            }
            if (S.lo[h] <= c && c <= S.hi[h]) { accepted = true; ws = ((ip - 1) & ~(W - 1)) + 1; we = ws + W - 1; break; }
        }
        left = c; right = 0;
        h0 = h;                                   // the loop below continues above the window counted here
        prev_ws = wsP; prev_we = wsP + PW - 1;
        __syncthreads();                          // sBk is reused by the next call
    }
    for (int64_t h = h0; !accepted && h <= S.height; ++h) {
        const int64_t W = S.seg << h;
        ws = ((ip - 1) & ~(W - 1)) + 1;
        we = ws + W - 1;
        left += blk_count(S, ws, prev_ws);
        right += blk_count(S, prev_we + 1, we + 1);
        const int64_t c = left + right;
        if (S.lo[h] <= c && c <= S.hi[h]) { accepted = true; break; }
        prev_ws = ws; prev_we = we;
    }
    const int64_t count = left + right;
    if (!accepted) {
        const int64_t H = S.height;
        if (count > S.hi[H] || (count < S.lo[H] && S.height > 1)) {
            __syncthreads();
            if (threadIdx.x == 0) {
                if (how == 0) occ_clear(S, ip);
                else if (how == 1) occ_clear(S, pe);
                else if (how == 2) occ_clear(S, cap);
                else { occ_clear(S, pe); occ_set(S, cap - 1); occ_clear(S, cap); }
            }
            __syncthreads();
            return false;
        }
        ws = 1; we = cap;
    }
    S.nb_elements += 1;
    const int64_t W = we - ws + 1;
    if (W == S.seg) { L = ip; return true; }
    S.stat_rebalances += 1; S.stat_window_slots += W;
    if (W <= SMALL_W) S.stat_small += 1;
    blk_rewrite_bits(S, ws, we, count);
    L = ws - 1 + spread_last_cell(make_geom(W, count));
    return true;
}

// Expands the ops of a MappedPackedCSC run into its cell stream (a semaphore cell (0, id) in front of the first row of every
// new column), appends the new columns to col_keys / col_live and writes one type bit per cell.  One workgroup.
__global__ __launch_bounds__(1024) void k_run_expand(const Op* ops, int64_t i0, int64_t R, const Ctl* ctl, int64_t* col_keys,
                                                     uint8_t* col_live, Op* cells, uint64_t* flags, int64_t* out) {
    __shared__ uint32_t wsum[16];
    __shared__ uint32_t carry_s;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t tl0 = ctl->table_len;
    const int64_t lastcol = tl0 > 0 ? col_keys[tl0 - 1] : 0;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (int64_t base = 0; base < R; base += 1024) {
        const int64_t j = base + tid;
        Op o; o.a = 0; o.b = 0; o.v = 0.0; o.kind = 0; o.pad = 0;
        uint32_t newc = 0;
        if (j < R) {
            o = ops[i0 + j];
            newc = (j == 0) ? ((tl0 == 0 || o.b != lastcol) ? 1u : 0u) : (o.b != ops[i0 + j - 1].b ? 1u : 0u);
        }
        const uint32_t ex = wave_excl_scan(newc);
        if (lane == 63) wsum[wv] = ex + newc;
        __syncthreads();
        uint32_t woff = 0;
        for (int k = 0; k < wv; ++k) woff += wsum[k];
        const uint32_t carry = carry_s;
        const int64_t before = (int64_t)carry + woff + ex;          // new columns in front of op j
        if (j < R) {
            const int64_t c0 = j + before;
            Op cell; cell.b = 0; cell.kind = 0; cell.pad = 0;
            if (newc) {
                cell.a = SEM_KEY; cell.v = (double)(tl0 + before + 1);
                cells[c0] = cell;
                col_keys[tl0 + before] = o.b; col_live[tl0 + before] = 1;
            }
            cell.a = o.a; cell.v = o.v;
            cells[c0 + newc] = cell;
        }
        __syncthreads();
        if (tid == 1023) carry_s = carry + woff + ex + newc;
        __syncthreads();
    }
    const int64_t T = R + (int64_t)carry_s;
    __threadfence_block();
    __syncthreads();
    for (int64_t base = 0; base < T; base += 1024) {
        const int64_t c = base + tid;
        const bool sem = c < T && cells[c].a == SEM_KEY;
        const uint64_t b = __ballot(sem);
        if (lane == 0) flags[(base >> 6) + wv] = b;
    }
    if (tid == 0) { out[0] = T; out[1] = (int64_t)carry_s; }
}

hipError_t launch_run_expand(const Op* ops, int64_t i0, int64_t R, const Ctl* ctl, int64_t* col_keys, uint8_t* col_live, Op* cells,
                             uint64_t* flags, int64_t* out, hipStream_t stream) {
    hipLaunchKernelGGL(k_run_expand, dim3(1), dim3(1024), 0, stream, ops, i0, R, ctl, col_keys, col_live, cells, flags, out);
    return hipGetLastError();
}

// The run itself is its own single-workgroup kernel (own register allocation: the per-op loop of wave 0 must stay
// spill-free).  Replays ops [i0, i0+R) on the bitmap `occ` (the saved copy for K-permute was made by the host) and
// updates the control block: next_op, nb_elements, statistics.  A run ends early at an op that needs _extend! /
// _shrink!; when that is the very first op, no_run_at tells the sequencer to execute it on the normal path.
__global__ __launch_bounds__(SEQ_BLOCK) void k_append_run(uint64_t* occ, Ctl* ctl, int64_t i0, int64_t R, const uint64_t* flags,
                                                          const int64_t* d_T, int wide_pos, int no_model, uint64_t* saved_memo,
                                                          const int64_t* m3_out) {
    __shared__ int64_t sRed[SEQ_BLOCK / 64];
    __shared__ RunComm sRun;
    extern __shared__ __attribute__((aligned(16))) unsigned char run_lds[];
    RunMemo& sMemo = *reinterpret_cast<RunMemo*>(run_lds);
    __shared__ int64_t sLo[MAX_LEVELS], sHi[MAX_LEVELS];
    // The memo is a pure function of the array's geometry (capacity, segment size, the integer thresholds of every level) and of
    // the kind of run: it survives from one run of the handle to the next in HBM (config 5: 50 runs of 17 000 cells on the same
    // geometry; a cold memo re-learns ~3000 (last word, cell types) epochs from the 1000 semaphores of each run) and is dropped
    // when the tag — a hash of exactly those inputs — changes (_extend!).
    uint64_t memo_tag = 0xcbf29ce484222325ull ^ (uint64_t)ctl->capacity;
    memo_tag = (memo_tag * 0x100000001b3ull) ^ (uint64_t)ctl->segment_capacity;
    memo_tag = (memo_tag * 0x100000001b3ull) ^ (uint64_t)(flags != nullptr ? 2 : 1);
    for (int h = 0; h <= (int)ctl->height && h < MAX_LEVELS; ++h) {
        memo_tag = (memo_tag * 0x100000001b3ull) ^ (uint64_t)ctl->lo[h];
        memo_tag = (memo_tag * 0x100000001b3ull) ^ (uint64_t)ctl->hi[h];
    }
    constexpr int MEMO_U4 = (int)(sizeof(RunMemo) / 16);
    static_assert(sizeof(RunMemo) % 16 == 0, "the memo is saved in 16-byte pieces");
    // the count-only replay (appendmodel.hip: k_append_model3, launched in front of this kernel) has placed the first m3_idx cells
    // on the bitmap and counted them in the control block; m3_ended: it stopped in front of an op that no level accepts
    const int64_t m3_idx = (m3_out != nullptr && m3_out[1] != 0) ? m3_out[0] : 0;
    const bool m3_ended = m3_out != nullptr && m3_out[1] == 2;
    const int64_t end_cells = flags != nullptr ? d_T[0] : R;
    const bool m3_all = m3_ended || (m3_out != nullptr && m3_out[1] != 0 && m3_idx >= end_cells);      // nothing left for this kernel's replay
    const bool memo_warm = !m3_all && saved_memo != nullptr && saved_memo[2 * MEMO_U4] == memo_tag;
    if (m3_all) {
    } else if (memo_warm) {
        const uint4* src = reinterpret_cast<const uint4*>(saved_memo);
        uint4* dst = reinterpret_cast<uint4*>(run_lds);
        for (int k = threadIdx.x; k < MEMO_U4; k += SEQ_BLOCK) dst[k] = src[k];
    } else {
        for (int k = threadIdx.x; k < MEMO_WORDS; k += SEQ_BLOCK) sMemo.words[k] = 0ull;      // 0 = entry not computed yet
        for (int k = threadIdx.x; k < M2_EV; k += SEQ_BLOCK) { sMemo.m2e[k].cnt = 0ull; sMemo.m2e[k].epr = ~0ull << 32; }
        for (int k = threadIdx.x; k < M2_HASH; k += SEQ_BLOCK) { sMemo.m2h[k].key = 0ull; sMemo.m2h[k].epr = 0ull; }
    }
    SeqBits S;
    S.occ = occ; S.ctl = ctl; S.sRed = sRed;
    S.capacity = ctl->capacity; S.seg = ctl->segment_capacity; S.height = ctl->height; S.nb_elements = ctl->nb_elements;
    S.stat_window_slots = ctl->stat_window_slots; S.stat_rebalances = ctl->stat_rebalances;
    S.stat_small = ctl->stat_small_rebalances;
    if (threadIdx.x < MAX_LEVELS) { sLo[threadIdx.x] = ctl->lo[threadIdx.x]; sHi[threadIdx.x] = ctl->hi[threadIdx.x]; }
    S.lo = sLo; S.hi = sHi;
    __syncthreads();
    RunComm* rc = &sRun;
    // cells of the run: the ops themselves (vector), or the expanded cell stream of k_run_expand (flags != nullptr)
    int64_t idx = m3_idx, L = d_prev_occupied(occ, S.capacity, 1);
    const int64_t end = end_cells;
    int64_t t_fast = 0, t_slow = 0, n_slow = 0;
    const bool narrow_pos = !wide_pos && S.capacity <= (1ll << 30) && end <= (1ll << 30);
    const int64_t c_begin = clock64(), w_begin = wall_clock64();
    const bool use_v2 = no_model == 0 && S.capacity >= RUN_BLOCK;
    if (threadIdx.x == 0) { sMemo.m2.outside_valid = 0; sMemo.m2.pending = 0; }
    __syncthreads();
    while (idx < end && !m3_ended) {
        if (use_v2 && !sMemo.m2.outside_valid) {
            // model v2: suffix cell counts of the levels wider than the block, without the last block (all threads, uniform)
            for (int j = 0; j <= (int)S.height && j < 64; ++j) {
                const int64_t W = S.seg << j;
                if (W > RUN_BLOCK && W <= S.capacity) {
                    const int64_t c = blk_count(S, S.capacity - W + 1, S.capacity - RUN_BLOCK + 1);
                    if (threadIdx.x == 0) sMemo.m2.outside[j] = (uint32_t)c;
                }
            }
            __syncthreads();
            if (threadIdx.x == 0) sMemo.m2.outside_valid = 1;
        }
        if (threadIdx.x == 0) { rc->idx = idx; rc->L = L; rc->pad = no_model; }
        __syncthreads();
        const int64_t t0 = wall_clock64();
        if (threadIdx.x < 64) {
            if (narrow_pos) wave_fast_appends<int32_t>(S, rc, &sMemo, flags, end);
            else wave_fast_appends<int64_t>(S, rc, &sMemo, flags, end);
        }
        __syncthreads();
        const int64_t t1 = wall_clock64();
        t_fast += t1 - t0;
        const int64_t nidx = rc->idx;
        L = rc->L;
        S.nb_elements += nidx - idx;
        S.stat_rebalances += rc->reb; S.stat_window_slots += rc->slots; S.stat_small += rc->small;
        idx = nidx;
        const int need = rc->need;
        __syncthreads();
        if (sMemo.m2.pending) {
            // model v2 left with rebalances wider than the block: the workgroup writes them, widest first, then wave 0 the rest
            for (int j = (int)S.height; j >= 0; --j) {
                const int64_t W = S.seg << j;
                if (W > RUN_BLOCK && W <= S.capacity && sMemo.m2.ev_valid[j] != 0) blk_rewrite_bits(S, S.capacity - W + 1, S.capacity, (int64_t)sMemo.m2.ev_c[j]);
            }
            __syncthreads();
            if (threadIdx.x < 64) wave_apply_inblock(S, &sMemo);
            __syncthreads();
            if (threadIdx.x == 0) { sMemo.m2.pending = 0; sMemo.m2.outside_valid = 0; }
            __syncthreads();
        }
        if (need != 1) continue;
        if (threadIdx.x == 0) sMemo.m2.outside_valid = 0;      // (the slow op changes the bitmap in front of the block)
        const bool ok = blk_slow_append(S, L, flags != nullptr && ((flags[idx >> 6] >> (idx & 63)) & 1ull));
        t_slow += wall_clock64() - t1; ++n_slow;
        if (!ok) break;
        ++idx;
    }
    // semaphore cells among the idx cells that were placed: new partitions; the others are completed ops
    int64_t nsem = 0;
    if (flags != nullptr) {
        for (int64_t wd = threadIdx.x; (wd << 6) < idx; wd += SEQ_BLOCK) {
            uint64_t f = flags[wd];
            if (((wd + 1) << 6) > idx) f &= mask_lt((int)(idx - (wd << 6)));
            nsem += popc64(f);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) nsem += __shfl_xor(nsem, o, 64);
        __syncthreads();
        if ((threadIdx.x & 63) == 0) sRed[threadIdx.x >> 6] = nsem;
        __syncthreads();
        nsem = 0;
        for (int k = 0; k < SEQ_BLOCK / 64; ++k) nsem += sRed[k];
    }
    if (saved_memo != nullptr && !m3_all) {
        __syncthreads();
        const uint4* src = reinterpret_cast<const uint4*>(run_lds);
        uint4* dst = reinterpret_cast<uint4*>(saved_memo);
        for (int k = threadIdx.x; k < MEMO_U4; k += SEQ_BLOCK) dst[k] = src[k];
        if (threadIdx.x == 0) saved_memo[2 * MEMO_U4] = memo_tag;
    }
    if (threadIdx.x == 0) {
        const int64_t next = i0 + idx - nsem;
        ctl->next_op = next;
        ctl->no_run_at = idx < end ? next : -1;
        ctl->nb_partitions += nsem; ctl->table_len += nsem;
        ctl->nb_elements = S.nb_elements;
        ctl->stat_window_slots = S.stat_window_slots; ctl->stat_rebalances = S.stat_rebalances;
        ctl->stat_small_rebalances = S.stat_small;
        ctl->dbg[0] = n_slow; ctl->dbg[2] = t_fast; ctl->dbg[3] = t_slow; ctl->dbg[4] = idx;
        ctl->dbg[1] = clock64() - c_begin; ctl->dbg[5] = wall_clock64() - w_begin;
    }
}

size_t append_run_memo_bytes() { return sizeof(RunMemo) + 16; }

hipError_t launch_append_run(uint64_t* occ, Ctl* ctl, int64_t i0, int64_t R, const uint64_t* flags, const int64_t* d_T,
                             uint64_t* saved_memo, const int64_t* m3_out, hipStream_t stream) {
    static const int wide_pos = [] { const char* e = dev_env("DSA_POS_WIDE"); return (e && e[0] == '1') ? 1 : 0; }();   // dev knob: 64-bit positions
    // dev knob DSA_COUNT_MODEL=0: bitmap replay only (the general per-op path; A/B runs and coverage of that path)
    static const int no_model = [] { const char* e = dev_env("DSA_COUNT_MODEL"); return (e && e[0] == '0') ? 1 : 0; }();
    static PerDeviceOnce once;
    {
        hipError_t e = once.run([] {
            return hipFuncSetAttribute(reinterpret_cast<const void*>(k_append_run), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(RunMemo));
        });
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_append_run, dim3(1), dim3(SEQ_BLOCK), sizeof(RunMemo), stream, occ, ctl, i0, R, flags, d_T, wide_pos, no_model, saved_memo, m3_out);
    return hipGetLastError();
}

}  // namespace dsa
