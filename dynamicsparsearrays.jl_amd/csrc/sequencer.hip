// csrc/sequencer.hip — the on-device write sequencer (K-find, K-shift, K-density, small-window
// K-rebalance) for gfx950.
//
// The reference has no batched insert: every setindex! depends on the slot layout left by the
// previous one (src/pma.jl:196-213, src/pcsr.jl:294-351).  A batch is therefore DEFINED as "apply the
// reference's setindex! in order", and one persistent 256-thread workgroup executes the whole batch
// on the device so that no host round trip is paid per element.  The control flow is executed
// redundantly and uniformly by all threads (same loads, same decisions); the data-moving steps are
// workgroup-parallel primitives:
//     d_find              exact emulation of the gap-tolerant bisection  src/finds.jl:29-57
//     blk_shift_right/left   _movecellstoright!/left! incl. semaphore fix-up  src/moves.jl:7-85
//     d_look_for_rebalance   density-threshold scan on the occupancy bitmap (popcounts) with the
//                            integer thresholds of Ctl  src/pma.jl:105-141, src/utils.jl:48-58
//     blk_rebalance_small    pack! + spread! of a window <= 8192 slots through LDS: ballot-style
//                            prefix popcounts compact the cells, closed-form gap offsets place them
//                            (src/moves.jl:94-171)
// Windows larger than that, _extend! / _shrink!, and table growth are handed back to the host
// ("yield"), which runs the grid-wide kernel of rebalance.hip and relaunches the sequencer.
// Also here: the detection of append runs (their bitmap replay is appendrun.hip), k_op_breaks / k_make_ops, and the parity hook
// k_dbg_raw, which runs the sequencer's primitives.  The read paths (lookups, checker, views) are in read.hip.
#include "seq_dev.h"

namespace dsa {

// dev profile of the sequencer (Ctl::prof, printed under DSA_DBG_TIME): compiled in with -DDSA_PROFILE only — the shader-clock
// reads (s_memtime) cost a few percent of a sequential op
#ifdef DSA_PROFILE
#define DSA_TICK() ((int64_t)__builtin_readcyclecounter())
#else
#define DSA_TICK() ((int64_t)0)
#endif

// result of one op: 0 = finished, otherwise a SeqStatus; RERUN is OR-ed in when the op must be
// executed again from the top after the host has serviced the yield
constexpr int RERUN = 0x100;

struct Seq : SeqBits {             // (occupancy words, geometry, density bounds, counters: seq_dev.h)
    KeyArr keys; double* vals;
    int64_t* sems; int64_t* col_keys; uint8_t* col_live;
    int64_t nb_partitions, table_len, table_cap;
    int64_t y_ws, y_we, y_m;
    int32_t err;
    bool tail_hint;                // the previous insert went behind the last cell of its range: try that first (append runs)
    const uint64_t* breaks;        // one bit per op of the batch (k_op_breaks): op j does not continue an append run from op j-1; may be null
    int64_t* sK; double* sV;       // LDS staging for the small-window rebalance
    uint32_t* sWordOff;            // [SMALL_W/64 + 1]
    // pending partitions (see "deferred column-table inserts" below): table entries [n_sorted, table_len) were created
    // in this launch at the END of the tables, in arrival order; pKey / pIdx (LDS) list them sorted by key
    int64_t n_sorted;
    int n_pend;
    int64_t prof[16];
    int64_t* pKey; uint32_t* pIdx; uint32_t* pLb;      // pLb: number of SORTED keys below the pending key
};
constexpr int PEND_MAX = TABLE_PEND_MAX;
static_assert(PEND_MAX % SEQ_BLOCK == 0, "d_import_pending distributes the list over the workgroup");


// ---- workgroup-parallel primitives ------------------------------------------------------------------

// cells [a, b-1] move one slot to the right (b is empty)  _moverightloop!  src/moves.jl:16-42
__device__ void blk_shift_right(Seq& S, int64_t a, int64_t b) {
    for (int64_t hi = b - 1; hi >= a; hi -= SEQ_BLOCK) {
        const int64_t p = hi - threadIdx.x;
        const bool act = p >= a;
        int64_t k = 0; double v = 0.0;
        if (act) { k = S.keys[p - 1]; v = S.vals[p - 1]; }
        __syncthreads();
        if (act) {
            S.keys[p] = k; S.vals[p] = v;
            if (S.sems != nullptr && k == SEM_KEY) S.sems[(int64_t)v - 1] = p + 1;
        }
        __syncthreads();
    }
}
// cells [a+1, b] move one slot to the left (a is empty); the cell at b may itself be empty
// (last_occ == false)  _moveleftloop!  src/moves.jl:59-85
__device__ void blk_shift_left(Seq& S, int64_t a, int64_t b, bool last_occ) {
    for (int64_t lo = a + 1; lo <= b; lo += SEQ_BLOCK) {
        const int64_t p = lo + threadIdx.x;
        const bool act = p <= b && (p < b || last_occ);
        int64_t k = 0; double v = 0.0;
        if (act) { k = S.keys[p - 1]; v = S.vals[p - 1]; }
        __syncthreads();
        if (act) {
            S.keys[p - 2] = k; S.vals[p - 2] = v;
            if (S.sems != nullptr && k == SEM_KEY) S.sems[(int64_t)v - 1] = p - 1;
        }
        __syncthreads();
    }
}

// pack! + spread! of [ws, we] (W <= SMALL_W) holding m cells  src/moves.jl:94-171
__device__ void blk_rebalance_small(Seq& S, int64_t ws, int64_t we, int64_t m) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t W = we - ws + 1;
    const int64_t lo0 = ws - 1;
    const int64_t w0 = lo0 >> 6;
    const SpreadGeom g = make_geom(W, m);
    if (W >= 64) {
        const int nwords = (int)(W >> 6);              // <= 128
        // exclusive prefix of the per-word popcounts: wave 0, 64 words per pass (any workgroup size)
        if (wv == 0) {
            uint32_t carry = 0;
            for (int g0 = 0; g0 < nwords; g0 += 64) {
                const int w = g0 + lane;
                const uint32_t pc = w < nwords ? (uint32_t)popc64(S.occ[w0 + w]) : 0u;
                const uint32_t ex = wave_excl_scan(pc);
                if (w < nwords) S.sWordOff[w] = carry + ex;
                carry += __shfl(ex + pc, 63, 64);
            }
        }
        __syncthreads();
        for (int w = wv; w < nwords; w += SEQ_BLOCK / 64) {
            const uint64_t mask = S.occ[w0 + w];
            if ((mask >> lane) & 1ull) {
                const uint32_t r = S.sWordOff[w] + (uint32_t)popc64(mask & mask_lt(lane));
                const int64_t s = ((w0 + w) << 6) + lane;
                S.sK[r] = S.keys[s];
                S.sV[r] = S.vals[s];
            }
        }
        __syncthreads();
        for (int64_t base = 0; base < W; base += SEQ_BLOCK) {
            const int q = (int)base + tid + 1;         // 1-based offset; W is a multiple of 64, block covers 4 words
            bool occd = false;
            if (q <= W) {
                int rank;
                if (!slot_is_gap(g, q, &rank)) {
                    occd = true;
                    const int64_t k = S.sK[rank - 1];
                    const double v = S.sV[rank - 1];
                    S.keys[lo0 + q - 1] = k;
                    S.vals[lo0 + q - 1] = v;
                    if (S.sems != nullptr && k == SEM_KEY) S.sems[(int64_t)v - 1] = lo0 + q;
                }
            }
            const uint64_t b = __ballot(occd);
            if (lane == 0 && base + wv * 64 < W) S.occ[w0 + ((base + wv * 64) >> 6)] = b;
        }
    } else {
        // the window lives inside one occupancy word; wave 0 handles it
        const int bit0 = (int)(lo0 & 63);
        const uint64_t wmask = ((1ull << W) - 1ull) << bit0;
        const uint64_t word = S.occ[w0];
        __syncthreads();                                // everyone has read the old word
        if (wv == 0) {
            const uint64_t mask = (word & wmask) >> bit0;
            if (lane < W && ((mask >> lane) & 1ull)) {
                const int r = popc64(mask & mask_lt(lane));
                S.sK[r] = S.keys[lo0 + lane];
                S.sV[r] = S.vals[lo0 + lane];
            }
            // single wave: LDS writes above are visible to the same wave after the implicit wave sync
            __builtin_amdgcn_s_waitcnt(0xc07f);        // lgkmcnt(0)
            bool occd = false;
            const int q = lane + 1;
            if (q <= W) {
                int rank;
                if (!slot_is_gap(g, q, &rank)) {
                    occd = true;
                    const int64_t k = S.sK[rank - 1];
                    const double v = S.sV[rank - 1];
                    S.keys[lo0 + q - 1] = k;
                    S.vals[lo0 + q - 1] = v;
                    if (S.sems != nullptr && k == SEM_KEY) S.sems[(int64_t)v - 1] = lo0 + q;
                }
            }
            const uint64_t b = __ballot(occd);
            if (lane == 0) S.occ[w0] = (word & ~wmask) | (b << bit0);
        }
    }
    __syncthreads();
    S.stat_small += 1;
}

// ---- the density-threshold scan  _look_for_rebalance!  src/pma.jl:105-141 -------------------------------
// returns 0 (nothing more to do) or a yield status
__device__ int d_after_count_change(Seq& S, int64_t pos) {
    int64_t prev_ws = pos, prev_we = pos - 1;
    int64_t left = 0, right = 0;
    int64_t ws = 1, we = S.capacity;
    bool accepted = false;
    int64_t h0 = 0;
    if (S.seg <= 64) {
        // the levels whose window fits the occupancy word of `pos` (windows are aligned powers of two): one load, popcounts of
        // sub-masks.  Only left + right is ever used, so the last window's count seeds `left` for the wider levels.
        const uint64_t word = S.occ[(pos - 1) >> 6];
        for (; h0 <= S.height; ++h0) {
            const int64_t W = S.seg << h0;
            if (W > 64) break;
            const int64_t ws0 = ((pos - 1) / W) * W;                          // 0-based first slot of the window
            const uint64_t mask = (W == 64 ? ~0ull : ((1ull << W) - 1ull)) << (ws0 & 63);
            const int64_t c = popc64(word & mask);
            ws = ws0 + 1; we = ws0 + W;
            left = c; right = 0;
            if (S.lo[h0] <= c && c <= S.hi[h0]) { accepted = true; break; }
            prev_ws = ws; prev_we = we;
        }
    }
    for (int64_t h = h0; !accepted && h <= S.height; ++h) {
        const int64_t W = S.seg << h;
        ws = ((pos - 1) / W) * W + 1;
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
        if (count > S.hi[H]) { S.y_m = count; return SEQ_Y_EXTEND; }
        if (count < S.lo[H] && S.height > 1) { S.y_m = count; return SEQ_Y_SHRINK; }
        ws = 1; we = S.capacity;
    }
    // _even_rebalance!  src/pma.jl:94-103 / src/pcsr.jl:88-97
    const int64_t W = we - ws + 1;
    if (W == S.seg) return 0;
    S.stat_rebalances += 1; S.stat_window_slots += W;
    if (W <= SMALL_W) { const int64_t tr0 = DSA_TICK(); blk_rebalance_small(S, ws, we, count); S.prof[12] += DSA_TICK() - tr0; S.prof[13] += 1; S.prof[14] += W; return 0; }
    S.y_ws = ws; S.y_we = we; S.y_m = count;
    return SEQ_Y_REBALANCE;
}

// number of leading ops of ops[i..n) that continue an append run.
//   mode 0 (vector):           OP_VEC_SET, non-zero value, key above the previous key (pa0 for the first op)
//   mode 1 (MappedPackedCSC):  OP_MPCSC_SET, non-zero value, row >= 1, (col, row) lexicographically above the previous
//                              (col, row) ((pb0, pa0) for the first op; any column when first_any)
__device__ int64_t blk_run_length(Seq& S, const Op* ops, int64_t i, int64_t n, int mode, int64_t pa0, int64_t pb0, bool first_any) {
    if (S.breaks != nullptr) {
        // op i against the state of the array, the ops behind it from the bitmap of the batch (one grid-wide pass when the ops were
        // uploaded: k_op_breaks) — the scan of 100 k ops by this one workgroup took 0.4 ms per detection
        const Op o = ops[i];
        const bool bad0 = mode == 0 ? !(o.kind == OP_VEC_SET && o.v != 0.0 && o.a > pa0)
                                    : !(o.kind == OP_MPCSC_SET && o.v != 0.0 && o.a >= 1 && (first_any || o.b > pb0 || (o.b == pb0 && o.a > pa0)));
        if (bad0) return 0;
        const int64_t w0 = (i + 1) >> 6, w1 = (n - 1) >> 6;          // bits i+1 .. n-1 (bits >= the batch length are set)
        for (int64_t base = w0; base <= w1; base += SEQ_BLOCK) {
            const int64_t w = base + threadIdx.x;
            uint64_t x = w <= w1 ? S.breaks[w] : 0ull;
            if (w == w0) x &= ~mask_lt((int)((i + 1) & 63));
            int64_t first = x ? (w << 6) + __ffsll((unsigned long long)x) - 1 : INT64_MAX;
#pragma unroll
            for (int o2 = 32; o2 > 0; o2 >>= 1) { const int64_t y = __shfl_xor(first, o2, 64); first = y < first ? y : first; }
            __syncthreads();
            if ((threadIdx.x & 63) == 0) S.sRed[threadIdx.x >> 6] = first;
            __syncthreads();
            first = S.sRed[0];
#pragma unroll
            for (int k = 1; k < SEQ_BLOCK / 64; ++k) first = S.sRed[k] < first ? S.sRed[k] : first;
            if (first != INT64_MAX) return (first < n ? first : n) - i;
        }
        return n - i;
    }
    int64_t R = 0;
    for (int64_t base = i; base < n; base += SEQ_BLOCK) {
        const int64_t j = base + threadIdx.x;
        bool bad = false;
        if (j < n) {
            const Op o = ops[j];
            int64_t pa = pa0, pb = pb0;
            bool any = first_any;
            if (j != i) { const Op q = ops[j - 1]; pa = q.a; pb = q.b; any = false; }
            if (mode == 0) bad = !(o.kind == OP_VEC_SET && o.v != 0.0 && o.a > pa);
            else bad = !(o.kind == OP_MPCSC_SET && o.v != 0.0 && o.a >= 1 && (any || o.b > pb || (o.b == pb && o.a > pa)));
        }
        const uint64_t b = __ballot(bad);
        __syncthreads();
        if ((threadIdx.x & 63) == 0)
            S.sRed[threadIdx.x >> 6] = b ? (int64_t)((threadIdx.x & ~63) + __ffsll((unsigned long long)b) - 1) : (int64_t)SEQ_BLOCK;
        __syncthreads();
        int64_t first = SEQ_BLOCK;
#pragma unroll
        for (int k = 0; k < SEQ_BLOCK / 64; ++k) first = S.sRed[k] < first ? S.sRed[k] : first;
        const int64_t lim = (n - base) < SEQ_BLOCK ? (n - base) : (int64_t)SEQ_BLOCK;
        if (first < lim) return R + first;
        R += lim;
    }
    return R;
}

// one bit per op of a batch: set when op j does NOT continue an append run from op j-1 (the conditions of blk_run_length; bit 0 and the
// bits behind the last op are set).  Grid-wide, enqueued behind the upload of the ops.
__global__ __launch_bounds__(256) void k_op_breaks(const Op* ops, int64_t n, int mode, uint64_t* breaks) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool bad = true;
    if (j > 0 && j < n) {
        const Op o = ops[j], q = ops[j - 1];
        if (mode == 0) bad = !(o.kind == OP_VEC_SET && o.v != 0.0 && o.a > q.a);
        else bad = !(o.kind == OP_MPCSC_SET && o.v != 0.0 && o.a >= 1 && (o.b > q.b || (o.b == q.b && o.a > q.a)));
    }
    const uint64_t b = __ballot(bad);
    if ((threadIdx.x & 63) == 0) breaks[j >> 6] = b;
}
// the op array of a batch from the caller's columns (uploaded as they are): op k = (a[k], b ? b[k] : 0, v[k], kind)
__global__ __launch_bounds__(256) void k_make_ops(const int64_t* __restrict__ a, const int64_t* __restrict__ b, const double* __restrict__ v,
                                                  int32_t kind, int64_t n, Op* __restrict__ ops) {
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (int64_t)gridDim.x * 256) {
        Op o; o.a = a[k]; o.b = b != nullptr ? b[k] : 0; o.v = v[k]; o.kind = kind; o.pad = 0;
        ops[k] = o;
    }
}
hipError_t launch_make_ops(const int64_t* a, const int64_t* b, const double* v, int32_t kind, int64_t n, Op* ops, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_make_ops, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 65536)), dim3(256), 0, stream, a, b, v, kind, n, ops);
    return hipGetLastError();
}
hipError_t launch_op_breaks(const Op* ops, int64_t n, int mode, uint64_t* breaks, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_op_breaks, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, ops, n, mode, breaks);
    return hipGetLastError();
}

// Run detection (inside the sequencer): number of ops of ops[i..] that form an append run, or 0.
__device__ int64_t d_detect_append_run(Seq& S, const Op* ops, int64_t i, int64_t n_avail) {
    if (S.nb_elements < 1) return 0;
    const int64_t L0 = d_prev_occupied(S.occ, S.capacity, 1);
    if (L0 < 1) return 0;
    const int64_t lk = S.keys[L0 - 1];
    const int64_t R = blk_run_length(S, ops, i, n_avail, 0, lk, 0, false);
    return R >= RUN_MIN ? R : 0;
}
// MappedPackedCSC: (col, row) ascending above the last cell of the last partition — new columns are appended partitions
// (addpartition!(pcsc) src/pcsr.jl:99-112 via setindex! src/pcsr.jl:341-351), rows go behind the last cell.
__device__ int64_t d_detect_pcsc_run(Seq& S, const Op* ops, int64_t i, int64_t n_avail) {
    const int64_t tl = S.table_len;
    int64_t pa0 = 0, pb0 = 0;
    bool any = false;
    if (tl == 0) {
        if (S.nb_elements != 0) return 0;
        any = true;
    } else {
        if (!S.col_live[tl - 1]) return 0;                 // tombstones at the end of the table: addpartition!(pcsc, prev) paths
        const int64_t sp = S.sems[tl - 1];
        if (sp == 0) return 0;
        pb0 = S.col_keys[tl - 1];
        const int64_t L0 = d_prev_occupied(S.occ, S.capacity, 1);
        if (L0 < sp) return 0;
        const int64_t lk = L0 == sp ? 0 : S.keys[L0 - 1];
        pa0 = lk > 0 ? lk : 0;
    }
    const int64_t R = blk_run_length(S, ops, i, n_avail, 1, pa0, pb0, any);
    return R >= RUN_MIN ? R : 0;
}

// _insert!(array, key, value, pos, semaphores)  src/writes.jl:26-43 ; returns the insertion position or 0 (EFULL)
__device__ int64_t d_insert_after(Seq& S, int64_t key, double val, int64_t pos) {
    const int64_t ne = d_next_empty(S.occ, pos, S.capacity);
    const int64_t pe = ne != 0 ? 0 : d_prev_empty(S.occ, pos);
    const bool last_occ = (ne == 0 && pe != 0) ? occ_test(S.occ, pos) : true;
    if (ne != 0 && ne - (pos + 1) <= SEQ_BLOCK) {
        // common case, fused: one chunk.  bitmap reads + cell loads | barrier | cell stores + new cell + bitmap | barrier
        const int64_t p = ne - 1 - threadIdx.x;
        const bool act = p >= pos + 1;
        int64_t k = 0; double v = 0.0;
        if (act) { k = S.keys[p - 1]; v = S.vals[p - 1]; }
        __syncthreads();
        if (act) {
            S.keys[p] = k; S.vals[p] = v;
            if (S.sems != nullptr && k == SEM_KEY) S.sems[(int64_t)v - 1] = p + 1;
        }
        if (threadIdx.x == 0) { S.keys[pos] = key; S.vals[pos] = val; occ_set(S, ne); }
        __syncthreads();
        return pos + 1;
    }
    __syncthreads();                       // every thread has finished reading the bitmap
    if (ne != 0) {
        blk_shift_right(S, pos + 1, ne);
        if (threadIdx.x == 0) { S.keys[pos] = key; S.vals[pos] = val; occ_set(S, ne); }
        __syncthreads();
        return pos + 1;
    }
    if (pe == 0) { S.err = E_FULL; return 0; }
    blk_shift_left(S, pe, pos, last_occ);
    if (threadIdx.x == 0) {
        S.keys[pos - 1] = key; S.vals[pos - 1] = val;
        // occupancy after the shift: bits [pe, pos-1] take the old bits [pe+1, pos]; (pe, pos-1] were all ones
        if (pe < pos - 1) { occ_set(S, pe); if (!last_occ) occ_clear(S, pos - 1); }
        else if (last_occ) occ_set(S, pe);
        occ_set(S, pos);
    }
    __syncthreads();
    return pos;
}

// setindex!(pma, value, key)  src/pma.jl:196-213 restricted to [from, to] like insert!/delete! of
// src/writes.jl:14-23,57-63 ; del_from is the (possibly wider) range of the delete path (src/pcsr.jl:302-307)
__device__ int d_set_in_range(Seq& S, int64_t key, double val, int64_t from, int64_t to, int64_t del_from) {
    if (val != 0.0) {
        // append runs (ascending keys: Coluna's column streaming, BASELINE config 2 batch A): when the previous insert landed
        // behind the last cell of its range, look there first — find() returns that cell whenever its key is smaller
        DFound f;
        bool have = false;
        if (S.tail_hint && to >= from) {
            const int64_t lp = d_prev_occupied(S.occ, to, from);
            if (lp >= from) {
                const int64_t lk = S.keys[lp - 1];
                if (lk < key) { f = DFound{lp, lk, 0.0, true}; have = true; }
            }
        }
        const int64_t ts0 = DSA_TICK();
        if (!have) f = d_find_fast(S.keys, S.vals, S.occ, key, from, to);     // [from, to] never holds a semaphore
        S.prof[8] += DSA_TICK() - ts0;
        S.tail_hint = have || (f.has && f.pos >= from && f.key < key && d_next_occupied(S.occ, f.pos, to) == 0);
        if (f.has && f.key == key && from <= f.pos && f.pos <= to) {
            __syncthreads();
            if (threadIdx.x == 0) S.vals[f.pos - 1] = val;
            __syncthreads();
            return 0;
        }
        const int64_t ts1 = DSA_TICK();
        const int64_t ip = d_insert_after(S, key, val, f.pos);
        if (ip == 0) return SEQ_ERROR;
        S.nb_elements += 1;
        const int64_t ts2 = DSA_TICK();
        const int rr = d_after_count_change(S, ip);
        S.prof[9] += ts2 - ts1; S.prof[10] += DSA_TICK() - ts2;
        return rr;
    }
    // the delete range of a partition starts AT its semaphore (key 0, src/pcsr.jl:307): the wave-parallel search is
    // only equivalent for key > 0 there; otherwise replay the reference bisection probe for probe
    const bool sorted_ok = (S.sems == nullptr) || key > SEM_KEY;
    const DFound f = sorted_ok ? d_find_fast(S.keys, S.vals, S.occ, key, del_from, to)
                               : d_find(S.keys, S.vals, S.occ, key, del_from, to);
    if (f.has && f.key == key) {
        __syncthreads();
        if (threadIdx.x == 0) occ_clear(S, f.pos);
        __syncthreads();
        S.nb_elements -= 1;
        return d_after_count_change(S, f.pos);
    }
    return 0;
}

// addpartition!(pcsc)  src/pcsr.jl:99-112
__device__ int d_addpartition_append(Seq& S) {
    if (S.table_len + 1 > S.table_cap) return SEQ_Y_TABLE_GROW | RERUN;
    const int64_t sem_pos = S.capacity;
    S.nb_partitions += 1;
    __syncthreads();
    if (threadIdx.x == 0) S.sems[S.table_len] = sem_pos;
    __syncthreads();
    S.table_len += 1;
    const double sem_val = (double)S.table_len;
    const int64_t ip = d_insert_after(S, SEM_KEY, sem_val, sem_pos);
    if (ip == 0) return SEQ_ERROR;
    S.nb_elements += 1;
    const int r = d_after_count_change(S, ip);
    return r ? (r | RERUN) : 0;
}

// addcolumn! (src/pcsr.jl:148-169) + addpartition!(pcsc, prev) (src/pcsr.jl:114-146); col_keys may be null (plain PackedCSC)
__device__ int d_addpartition_middle(Seq& S, int64_t prev, bool with_col, int64_t col) {
    // prev = prev_sem_id = prev_col_pos ; the new partition gets id prev+1 (0-based table index prev)
    if (prev + 1 < 1 || prev + 1 > S.table_len) { S.err = E_BOUNDS; return SEQ_ERROR; }
    const int64_t target = S.sems[prev];
    int64_t sem_pos = 0;
    if (target == 0) {
        // addcolumn! stores the column key in the tombstoned slot BEFORE addpartition! looks for the next semaphore
        // (src/pcsr.jl:155-156,165): the key stays there when that lookup throws
        __syncthreads();
        if (with_col && threadIdx.x == 0) { S.col_keys[prev] = col; S.col_live[prev] = 1; }
        __syncthreads();
        const int64_t next = d_next_live_sem(S.sems, prev + 1, S.table_len);
        if (next == 0) { S.err = E_BOUNDS; return SEQ_ERROR; }      // semaphores[0] in the reference (App. A.6 (3))
        sem_pos = S.sems[next - 1] - 1;
    } else {
        if (S.table_len + 1 > S.table_cap) return SEQ_Y_TABLE_GROW | RERUN;
        // reference @assert !isnothing(moved_sem_pos) (src/pcsr.jl:132): no tombstone may be shifted
        int bad = 0;
        for (int64_t i = prev + threadIdx.x; i < S.table_len; i += SEQ_BLOCK) if (S.sems[i] == 0) bad = 1;
        if (__syncthreads_or(bad)) { S.err = E_ASSERT; return SEQ_ERROR; }
        sem_pos = target - 1;
        // shift tables one entry to the right from index prev, highest chunk first
        for (int64_t hi = S.table_len - 1; hi >= prev; hi -= SEQ_BLOCK) {
            const int64_t i = hi - threadIdx.x;
            const bool act = i >= prev;
            int64_t sp = 0, ck = 0; uint8_t lv = 0;
            if (act) { sp = S.sems[i]; if (with_col) { ck = S.col_keys[i]; lv = S.col_live[i]; } }
            __syncthreads();
            if (act) {
                S.sems[i + 1] = sp;
                if (with_col) { S.col_keys[i + 1] = ck; S.col_live[i + 1] = lv; }
                S.vals[sp - 1] = (double)(i + 2);       // the semaphore of id i+1 becomes id i+2
            }
            __syncthreads();
        }
        if (with_col && threadIdx.x == 0) { S.col_keys[prev] = col; S.col_live[prev] = 1; }
        S.table_len += 1;
    }
    __syncthreads();
    S.nb_partitions += 1;
    const double sem_val = (double)(prev + 1);
    const int64_t ip = d_insert_after(S, SEM_KEY, sem_val, sem_pos);
    if (ip == 0) return SEQ_ERROR;
    if (threadIdx.x == 0) S.sems[prev] = ip;
    __syncthreads();
    S.nb_elements += 1;
    const int r = d_after_count_change(S, ip);
    return r ? (r | RERUN) : 0;
}

// ---- deferred column-table inserts ----------------------------------------------------------------------------------
// addpartition!(pcsc, prev) in the middle of the tables (src/pcsr.jl:114-146) shifts semaphores[] / col_keys[] one entry to
// the right and rewrites the id stored in EVERY later semaphore cell: O(#partitions) per new column — the cost of streaming
// new rows into the rowmajor twin in random key order (BASELINE config 5: 100k rows -> 5e9 id rewrites).  Ids are only
// labels: the slot layout depends on WHERE the new semaphore cell is inserted (in front of the semaphore of its successor in
// key order), not on its number.  So inside one launch a new partition is appended at the END of the tables with the next
// free id (cells and tables stay consistent with each other: shifts, rebalances and spreads keep working on ids), its key
// is kept in a small sorted list in LDS, lookups consult the sorted table part + that list, and the tables are brought
// back to key order — ONE merge pass with ONE renumbering of the cells — when the list is full and before any op that is not
// a plain MappedPackedCSC write (d_merge_pending below, one workgroup), or by the host between launches and before the batch
// returns (tables.hip: the same pass with the whole chip; entries still pending when the kernel exits are counted in
// Ctl::n_pending and re-imported by the next launch; the big rebalance and the batch-parallel kernels work on ids and do not
// care about the order).  Only used while no tombstone exists (nb_partitions == table_len); the tombstone-reuse and @assert
// paths of the reference run on the literal code below.
__device__ int pend_lower_bound(const Seq& S, int64_t key) {          // first j with pKey[j] >= key
    int lo = 0, hi = S.n_pend;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (S.pKey[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}
__device__ void pend_insert(Seq& S, int64_t key, int64_t idx, int64_t lb, int p) {
    __syncthreads();
    int64_t kk[PEND_MAX / SEQ_BLOCK]; uint32_t ii[PEND_MAX / SEQ_BLOCK], ll[PEND_MAX / SEQ_BLOCK];
#pragma unroll
    for (int u = 0; u < PEND_MAX / SEQ_BLOCK; ++u) {
        const int j = p + threadIdx.x + SEQ_BLOCK * u;
        if (j < S.n_pend) { kk[u] = S.pKey[j]; ii[u] = S.pIdx[j]; ll[u] = S.pLb[j]; }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < PEND_MAX / SEQ_BLOCK; ++u) {
        const int j = p + threadIdx.x + SEQ_BLOCK * u;
        if (j < S.n_pend) { S.pKey[j + 1] = kk[u]; S.pIdx[j + 1] = ii[u]; S.pLb[j + 1] = ll[u]; }
    }
    if (threadIdx.x == 0) { S.pKey[p] = key; S.pIdx[p] = (uint32_t)idx; S.pLb[p] = (uint32_t)lb; }
    __syncthreads();
    S.n_pend += 1;
}
// successor in key order of `key` (which is in neither set, or is the key of partition `self`): 0-based table index, -1 if none.
// sorted_succ = 0-based index of the first sorted entry with a larger key (>= n_sorted: none)
__device__ int64_t succ_index(const Seq& S, int64_t sorted_succ, int64_t key) {
    const int pj = pend_lower_bound(S, key + 1);
    const bool has_s = sorted_succ < S.n_sorted, has_p = pj < S.n_pend;
    if (has_s && has_p) return S.col_keys[sorted_succ] < S.pKey[pj] ? sorted_succ : (int64_t)S.pIdx[pj];
    if (has_s) return sorted_succ;
    if (has_p) return (int64_t)S.pIdx[pj];
    return -1;
}
// tables back to key order: sorted entry i moves up by the number of pending keys below it, pending rank r goes to
// (#sorted keys below it) + r; every cell whose id changed is rewritten once
__device__ void d_merge_pending(Seq& S) {
    const int K = S.n_pend;
    if (K == 0) return;
    const int64_t tm0 = DSA_TICK();
    __syncthreads();
    const int64_t ns = S.n_sorted;
    int64_t* dst = S.sK;                                      // dynamic LDS is free between ops
    int64_t* spos = reinterpret_cast<int64_t*>(S.sV);
    for (int r = threadIdx.x; r < K; r += SEQ_BLOCK) {
        dst[r] = (int64_t)S.pLb[r] + r;                       // (#sorted keys below it) + (#pending keys below it)
        spos[r] = S.sems[S.pIdx[r]];
    }
    __syncthreads();
    const int64_t i_min = dst[0];                              // sorted entries below the smallest pending key stay
    constexpr int U = 4;
    for (int64_t hi = ns - 1; hi >= i_min; hi -= SEQ_BLOCK * U) {
        int64_t sp[U], ck[U]; int sh[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = hi - threadIdx.x - SEQ_BLOCK * u;
            if (i >= i_min) { sp[u] = S.sems[i]; ck[u] = S.col_keys[i]; }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = hi - threadIdx.x - SEQ_BLOCK * u;
            sh[u] = i >= i_min ? pend_lower_bound(S, ck[u]) : 0;
        }
        __syncthreads();               // all loads of the chunk before its stores; stores never reach below the chunk
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = hi - threadIdx.x - SEQ_BLOCK * u;
            if (i >= i_min && sh[u] > 0) {
                const int64_t d = i + sh[u];
                S.sems[d] = sp[u]; S.col_keys[d] = ck[u]; S.col_live[d] = 1;
                S.vals[sp[u] - 1] = (double)(d + 1);
            }
        }
    }
    __syncthreads();
    for (int r = threadIdx.x; r < K; r += SEQ_BLOCK) {
        const int64_t d = dst[r];
        S.sems[d] = spos[r]; S.col_keys[d] = S.pKey[r]; S.col_live[d] = 1;
        S.vals[spos[r] - 1] = (double)(d + 1);
    }
    __syncthreads();
    S.n_sorted = S.table_len;
    S.n_pend = 0;
    S.prof[3] += DSA_TICK() - tm0; S.prof[6] += 1;
}

// entries left at the end of the tables by earlier launches of the batch (Ctl::n_pending, arrival order: batch-parallel rounds and
// previous sequencer chunks): rebuild the sorted list; the merge itself is the host's grid-wide pass (tables.hip) or, when the
// list fills up inside this launch, d_merge_pending
__device__ void d_import_pending(Seq& S, int64_t K) {
    if (K <= 0) return;
    const int64_t ns = S.table_len - K;
    S.n_sorted = ns;
    int64_t* tmp = S.sK;                                       // dynamic LDS is free between ops
    for (int64_t r = threadIdx.x; r < K; r += SEQ_BLOCK) tmp[r] = S.col_keys[ns + r];
    __syncthreads();
    for (int64_t r = threadIdx.x; r < K; r += SEQ_BLOCK) {
        const int64_t key = tmp[r];
        int rank = 0;
        for (int64_t j = 0; j < K; ++j) rank += tmp[j] < key ? 1 : 0;          // keys are distinct
        int64_t lo = 0, hi = ns;
        while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (S.col_keys[mid] < key) lo = mid + 1; else hi = mid; }
        S.pKey[rank] = key; S.pIdx[rank] = (uint32_t)(ns + r); S.pLb[rank] = (uint32_t)lo;
    }
    __syncthreads();
    S.n_pend = (int)K;
}

// _pos_of_partition_end  src/pcsr.jl:177-186
__device__ int64_t d_partition_end(Seq& S, int64_t partition) {
    if (S.n_pend > 0) {            // no tombstones in this mode: the successor in key order, sorted part or pending list
        const int64_t kp = S.col_keys[partition - 1];
        int64_t sorted_succ = partition;                        // 0-based index of the next sorted entry
        if (partition > S.n_sorted) {
            const DFoundKey f = d_find_table_fast(S.col_keys, S.col_live, S.n_sorted, kp);
            sorted_succ = f.has ? f.pos : 0;                    // number of sorted keys < kp
        }
        const int64_t sidx = succ_index(S, sorted_succ, kp);
        return sidx >= 0 ? S.sems[sidx] - 1 : S.capacity;
    }
    const int64_t next = d_next_live_sem(S.sems, partition, S.table_len);
    return next != 0 ? S.sems[next - 1] - 1 : S.capacity;
}

// setindex!(pcsc, value, key, partition)  src/pcsr.jl:294-339
__device__ int d_pcsc_set(Seq& S, double val, int64_t key, int64_t partition) {
    if (partition < 1) { S.err = E_BOUNDS; return SEQ_ERROR; }
    while (partition > S.table_len) {                   // _add_partitions!  :312-319
        const int r = d_addpartition_append(S);
        if (r) return r;
    }
    const int64_t from = S.sems[partition - 1];
    if (from == 0) { S.err = E_DELETED; return SEQ_ERROR; }
    const int64_t te0 = DSA_TICK();
    const int64_t to = d_partition_end(S, partition);
    S.prof[11] += DSA_TICK() - te0;
    return d_set_in_range(S, key, val, from + 1, to, from);
}

// purge!(array, from, to)  src/writes.jl:80-91: clears every slot of [from, to]; returns the number of cells deleted
__device__ int64_t blk_purge(Seq& S, int64_t from, int64_t to) {
    if (to < from) return 0;
    const int64_t nb = blk_count(S, from, to + 1);
    __syncthreads();
    const int64_t lo0 = from - 1, hi0 = to - 1;
    const int64_t w0 = lo0 >> 6, w1 = hi0 >> 6;
    for (int64_t w = w0 + threadIdx.x; w <= w1; w += SEQ_BLOCK) S.occ[w] &= ~word_range_mask(w, lo0, hi0);
    __syncthreads();
    return nb;
}

// deletepartition!  src/pcsr.jl:188-204
__device__ int d_deletepartition(Seq& S, int64_t partition) {
    if (!(1 <= partition && partition <= S.table_len)) { S.err = E_BOUNDS; return SEQ_ERROR; }
    S.nb_partitions -= 1;
    const int64_t sem_pos = S.sems[partition - 1];
    if (sem_pos == 0) { S.err = E_ASSERT; return SEQ_ERROR; }
    const int64_t end = d_partition_end(S, partition);
    const int64_t nb = blk_purge(S, sem_pos, end);
    if (threadIdx.x == 0) S.sems[partition - 1] = 0;
    __syncthreads();
    const int64_t mid = sem_pos + (end - sem_pos) / 2;
    if (nb > 0) {
        S.nb_elements -= nb;
        return d_after_count_change(S, mid);
    }
    return 0;
}

__device__ int d_exec(Seq& S, const Op& op) {
    if (op.kind != OP_MPCSC_SET && S.n_pend > 0) d_merge_pending(S);
    switch (op.kind) {
        case OP_VEC_SET:
            return d_set_in_range(S, op.a, op.v, 1, S.capacity, 1);
        case OP_PCSC_SET:
            return d_pcsc_set(S, op.v, op.a, op.b);
        case OP_MPCSC_SET: {       // setindex!(mpcsc, value, row, col)  src/pcsr.jl:341-351
            if (S.n_pend == PEND_MAX) d_merge_pending(S);
            if (S.n_pend == 0) S.n_sorted = S.table_len;
            const int64_t tp0 = DSA_TICK();
            const bool no_tombstone = S.nb_partitions == S.table_len;
            const DFoundKey f = d_find_table_fast(S.col_keys, S.col_live, S.n_sorted, op.b, no_tombstone);
            int64_t col_pos = f.pos;
            bool found = f.has && f.key == op.b;
            int pj = 0;
            // successor of the column in key order (0-based table index, -1: none, -2: not known yet) — bounds its slot range
            int64_t sidx = -2;
            if (found && S.n_pend > 0) sidx = succ_index(S, col_pos, op.b);
            if (!found && S.n_pend > 0) {
                pj = pend_lower_bound(S, op.b);
                if (pj < S.n_pend && S.pKey[pj] == op.b) {
                    found = true; col_pos = (int64_t)S.pIdx[pj] + 1;
                    sidx = succ_index(S, (int64_t)S.pLb[pj], op.b);
                }
            }
            const int64_t tp1 = DSA_TICK();
            S.prof[0] += tp1 - tp0; S.prof[4] += 1;
            if (!found) {
                if (S.n_pend == 0 && (f.pos == S.table_len || !no_tombstone)) {
                    // the literal paths of the reference: append behind the last column, or middle insert with tombstones around
                    if (f.pos == S.table_len) {
                        if (S.table_len + 1 > S.table_cap) return SEQ_Y_TABLE_GROW | RERUN;
                        __syncthreads();
                        if (threadIdx.x == 0) { S.col_keys[S.table_len] = op.b; S.col_live[S.table_len] = 1; }
                        __syncthreads();
                        const int r = d_addpartition_append(S);
                        S.n_sorted = S.table_len;
                        if (r) return r;
                        col_pos = S.table_len;
                    } else {
                        const int r = d_addpartition_middle(S, f.pos, true, op.b);
                        S.n_sorted = S.table_len;
                        if (r) return r;
                        col_pos = f.pos + 1;
                    }
                } else {
                    // deferred middle insert: same semaphore cell at the same place, table entry at the end (see above)
                    if (S.table_len + 1 > S.table_cap) return SEQ_Y_TABLE_GROW | RERUN;
                    const int64_t lb = f.has ? f.pos : 0;
                    sidx = succ_index(S, lb, op.b);
                    const int64_t sem_pos = sidx >= 0 ? S.sems[sidx] - 1 : S.capacity;
                    const int64_t idx = S.table_len;
                    __syncthreads();
                    if (threadIdx.x == 0) { S.col_keys[idx] = op.b; S.col_live[idx] = 1; S.sems[idx] = sem_pos; }
                    __syncthreads();
                    S.table_len += 1;
                    S.nb_partitions += 1;
                    pend_insert(S, op.b, idx, lb, pj);
                    const int64_t ip = d_insert_after(S, SEM_KEY, (double)(idx + 1), sem_pos);
                    if (ip == 0) return SEQ_ERROR;
                    if (threadIdx.x == 0) S.sems[idx] = ip;
                    __syncthreads();
                    S.nb_elements += 1;
                    const int r = d_after_count_change(S, ip);
                    if (r) return r | RERUN;
                    col_pos = idx + 1;
                }
                S.prof[1] += DSA_TICK() - tp1; S.prof[5] += 1;
            }
            const int64_t tp2 = DSA_TICK();
            int rr;
            if (sidx == -2) rr = d_pcsc_set(S, op.v, op.a, col_pos);
            else {
                // setindex!(pcsc, value, key, partition) with the range end already known  src/pcsr.jl:294-310
                const int64_t from = S.sems[col_pos - 1];
                const int64_t to = sidx >= 0 ? S.sems[sidx] - 1 : S.capacity;
                rr = d_set_in_range(S, op.a, op.v, from + 1, to, from);
            }
            S.prof[2] += DSA_TICK() - tp2;
            return rr;
        }
        case OP_DELETE_PARTITION:
            return d_deletepartition(S, op.b);
        case OP_MPCSC_DELETECOLUMN: {   // deletecolumn!(mpcsc, col)  src/pcsr.jl:206-212
            const DFoundKey f = d_find_table_fast(S.col_keys, S.col_live, S.table_len, op.b);
            if (!(f.has && f.key == op.b)) { S.err = E_ARG; return SEQ_ERROR; }
            __syncthreads();
            if (threadIdx.x == 0) S.col_live[f.pos - 1] = 0;
            __syncthreads();
            return d_deletepartition(S, f.pos);
        }
        default:
            S.err = E_ARG;
            return SEQ_ERROR;
    }
}

// The state a kernel of this unit starts from: the slot arrays and the LDS staging it was given, no column tables, no control block,
// no pending list, every counter at zero.  The kernel then sets the geometry and whatever else it has.
__device__ __forceinline__ void seq_init(Seq& S, KeyArr keys, double* vals, uint64_t* occ, int64_t* sems, unsigned char* lds,
                                         uint32_t* sWordOff, int64_t* sRed) {
    S.keys = keys; S.vals = vals; S.occ = occ; S.sems = sems; S.col_keys = nullptr; S.col_live = nullptr; S.ctl = nullptr;
    S.nb_elements = 0; S.nb_partitions = 0; S.table_len = 0; S.table_cap = 0;
    S.stat_window_slots = S.stat_rebalances = S.stat_small = 0;
    S.y_ws = S.y_we = S.y_m = 0; S.err = 0; S.tail_hint = false; S.breaks = nullptr;
    S.n_sorted = 0; S.n_pend = 0; S.pKey = nullptr; S.pIdx = nullptr; S.pLb = nullptr;
    for (int q = 0; q < 16; ++q) S.prof[q] = 0;
    S.sK = reinterpret_cast<int64_t*>(lds);
    S.sV = reinterpret_cast<double*>(lds + SMALL_W * sizeof(int64_t));
    S.sWordOff = sWordOff; S.sRed = sRed; S.lo = nullptr; S.hi = nullptr;
}

__global__ __launch_bounds__(SEQ_BLOCK) void k_sequencer(KeyArr keys, double* vals, uint64_t* occ, int64_t* sems,
                                                         int64_t* col_keys, uint8_t* col_live, Ctl* ctl,
                                                         const Op* ops, int64_t n_ops, int64_t n_avail, int run_ok, const uint64_t* breaks,
                                                         Ctl* host_ctl, unsigned long long* host_seq, unsigned int seq) {
    // host_ctl / host_seq (pinned, may be null): the kernel hands its control block back itself — every word, then `seq` into the word the
    // host polls for — instead of a publish launch behind it (as parbatch.hip's k_publish does for a burst of rounds)
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ int64_t sRed[SEQ_BLOCK / 64];
    __shared__ uint32_t sWordOff[SMALL_W / 64 + 1];
    Seq S;
    seq_init(S, keys, vals, occ, sems, lds, sWordOff, sRed);
    S.col_keys = col_keys; S.col_live = col_live; S.ctl = ctl; S.breaks = breaks;
    S.capacity = ctl->capacity; S.seg = ctl->segment_capacity; S.height = ctl->height;
    S.nb_elements = ctl->nb_elements; S.nb_partitions = ctl->nb_partitions;
    S.table_len = ctl->table_len; S.table_cap = ctl->table_cap;
    S.stat_window_slots = ctl->stat_window_slots; S.stat_rebalances = ctl->stat_rebalances;
    S.stat_small = ctl->stat_small_rebalances;
    __shared__ int64_t sPKey[PEND_MAX];
    __shared__ uint32_t sPIdx[PEND_MAX];
    __shared__ uint32_t sPLb[PEND_MAX];
    S.n_sorted = S.table_len; S.pKey = sPKey; S.pIdx = sPIdx; S.pLb = sPLb;
    const int64_t tk0 = DSA_TICK();
    __shared__ int64_t sLo[MAX_LEVELS], sHi[MAX_LEVELS];
    if (threadIdx.x < MAX_LEVELS) { sLo[threadIdx.x] = ctl->lo[threadIdx.x]; sHi[threadIdx.x] = ctl->hi[threadIdx.x]; }
    S.lo = sLo; S.hi = sHi;
    __syncthreads();
    if (col_keys != nullptr && ctl->n_pending > 0) d_import_pending(S, ctl->n_pending);

    int64_t i = ctl->next_op;
    int status = SEQ_DONE;
    Op op = ops[i < n_ops ? i : 0];
    int64_t run_cooldown = 0;
    const int64_t no_run_at = ctl->no_run_at;
    for (; i < n_ops; ++i) {
        const Op nxt = ops[i + 1 < n_ops ? i + 1 : i];          // prefetched under the current op's memory traffic
        const bool vec_cand = sems == nullptr && op.kind == OP_VEC_SET && nxt.kind == OP_VEC_SET && nxt.a > op.a;
        const bool csc_cand = col_keys != nullptr && op.kind == OP_MPCSC_SET && nxt.kind == OP_MPCSC_SET &&
                              (nxt.b > op.b || (nxt.b == op.b && nxt.a > op.a));
        // (no detection while middle inserts are pending: an append run needs its columns behind the last key)
        if (run_ok && (vec_cand || csc_cand) && op.v != 0.0 && i + RUN_MIN <= n_avail && i != no_run_at && S.n_pend == 0 && --run_cooldown < 0) {
            const int64_t R = vec_cand ? d_detect_append_run(S, ops, i, n_avail) : d_detect_pcsc_run(S, ops, i, n_avail);
            if (R > 0) {
                S.y_ws = i; S.y_we = S.nb_elements; S.y_m = R;
                status = SEQ_Y_APPEND_RUN;
                break;
            }
            run_cooldown = 32;
        }
        const int r = d_exec(S, op);
        if (r != 0) {
            status = r & 0xff;
            if (!(r & RERUN) && status != SEQ_ERROR) ++i;      // the op itself is complete once the host has acted
            break;
        }
        op = nxt;
    }
    // pending entries stay at the end of the tables (Ctl::n_pending): the host merges them with the whole chip (tables.hip) when
    // enough have piled up and before the batch returns; the next launch re-imports what is left
    __syncthreads();
    if (threadIdx.x == 0) {
        ctl->next_op = i;
        ctl->status = status;
        ctl->err = S.err;
        ctl->err_op = (status == SEQ_ERROR) ? i : -1;
        ctl->nb_elements = S.nb_elements; ctl->nb_partitions = S.nb_partitions; ctl->table_len = S.table_len;
        ctl->n_pending = S.n_pend;
        ctl->y_ws = S.y_ws; ctl->y_we = S.y_we; ctl->y_m = S.y_m;
        ctl->stat_window_slots = S.stat_window_slots; ctl->stat_rebalances = S.stat_rebalances;
        ctl->stat_small_rebalances = S.stat_small;
        S.prof[7] = DSA_TICK() - tk0;
        for (int q = 0; q < 16; ++q) ctl->prof[q] += S.prof[q];
    }
    if (host_seq != nullptr) {
        __builtin_amdgcn_s_waitcnt(0);
        __syncthreads();                               // thread 0's words are on their way to the L2
        const unsigned long long* src = reinterpret_cast<const unsigned long long*>(ctl);
        unsigned long long* dst = reinterpret_cast<unsigned long long*>(host_ctl);
        for (int q = threadIdx.x; q < (int)(sizeof(Ctl) / 8); q += SEQ_BLOCK)
            __hip_atomic_store(dst + q, __hip_atomic_load(src + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __builtin_amdgcn_s_waitcnt(0);
        __syncthreads();
        if (threadIdx.x == 0) {
            publish_seq(host_seq, (unsigned long long)seq);
        }
    }
}

hipError_t launch_sequencer(KeyArr keys, double* vals, uint64_t* occ, int64_t* sems, int64_t* col_keys,
                            uint8_t* col_live, Ctl* ctl, const Op* ops, int64_t n_ops, int64_t n_avail, bool run_ok, const uint64_t* breaks,
                            Ctl* host_ctl, unsigned long long* host_seq, unsigned int seq, hipStream_t stream) {
    const size_t lds_bytes = (size_t)SMALL_W * (sizeof(int64_t) + sizeof(double));
    static PerDeviceOnce once;
    {
        hipError_t e = once.run([] {
            return hipFuncSetAttribute(reinterpret_cast<const void*>(k_sequencer), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        });
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_sequencer, dim3(1), dim3(SEQ_BLOCK), lds_bytes, stream, keys, vals, occ, sems, col_keys, col_live,
                       ctl, ops, n_ops, n_avail, run_ok ? 1 : 0, breaks, host_ctl, host_seq, seq);
    return hipGetLastError();
}

// ---- parity hooks (include/dsa.h: dsa_dbg_raw_*) ------------------------------------------------------------------------------
// The slot-array primitives of the sequencer run on a caller-supplied RAW slot array (any length, any content), so that the
// reference's own unit-test vectors (test/unit/finds.jl, test/unit/writes.jl) are checked on the device code itself and not only on
// the CPU oracle.  One workgroup, one op.  out[0] = error code, out[1] = position, out[2] = flag (element found / new key / deleted),
// out[3] = key of the element found, out[4] = its value (bits), out[5] = cells purged.
__global__ __launch_bounds__(SEQ_BLOCK) void k_dbg_raw(KeyArr keys, double* vals, uint64_t* occ, int64_t* sems, int64_t len, int op,
                                                       int64_t key, double val, int64_t from, int64_t to, int64_t m, int64_t* out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ int64_t sRed[SEQ_BLOCK / 64];
    __shared__ uint32_t sWordOff[SMALL_W / 64 + 1];
    Seq S;
    seq_init(S, keys, vals, occ, sems, lds, sWordOff, sRed);
    S.capacity = len; S.seg = 1; S.height = 0;
    int64_t r_pos = 0, r_flag = 0, r_key = 0, r_nb = 0; double r_val = 0.0;
    switch (op) {
        case DBG_FIND: case DBG_FIND_FAST: {                       // find(array, key, from, to)  src/finds.jl:29-57
            const DFound f = op == DBG_FIND ? d_find(keys, vals, occ, key, from, to) : d_find_fast(keys, vals, occ, key, from, to);
            r_pos = f.pos; r_flag = f.has ? 1 : 0; r_key = f.key; r_val = f.val;
            break;
        }
        case DBG_INSERT: case DBG_INSERT_FAST: {                   // insert!(array, key, value, from, to, semaphores)  src/writes.jl:14-43
            const DFound f = op == DBG_INSERT ? d_find(keys, vals, occ, key, from, to) : d_find_fast(keys, vals, occ, key, from, to);
            if (f.has && f.key == key && from <= f.pos && f.pos <= to) {
                __syncthreads();
                if (threadIdx.x == 0) vals[f.pos - 1] = val;
                r_pos = f.pos; r_flag = 0;
            } else {
                r_pos = d_insert_after(S, key, val, f.pos);
                r_flag = 1;
            }
            break;
        }
        case DBG_DELETE: case DBG_DELETE_FAST: {                   // delete!(array, key, from, to)  src/writes.jl:57-68
            const DFound f = op == DBG_DELETE ? d_find(keys, vals, occ, key, from, to) : d_find_fast(keys, vals, occ, key, from, to);
            if (f.has && f.key == key) {
                __syncthreads();
                if (threadIdx.x == 0) occ_clear(S, f.pos);
                r_pos = f.pos; r_flag = 1;
            }
            break;
        }
        case DBG_PURGE:                                            // purge!(array, from, to)  src/writes.jl:80-91
            if (to >= from) { r_nb = blk_purge(S, from, to); r_pos = from + (to - from) / 2; }
            break;
        case DBG_REBALANCE:                                        // pack! + spread! of [from, to] holding m cells  src/moves.jl:94-171
            blk_rebalance_small(S, from, to, m);
            break;
        default:
            S.err = E_ARG;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        out[0] = S.err; out[1] = r_pos; out[2] = r_flag; out[3] = r_key; out[4] = __double_as_longlong(r_val); out[5] = r_nb;
    }
}

hipError_t launch_dbg_raw_block(KeyArr keys, double* vals, uint64_t* occ, int64_t* sems, int64_t len, int op, int64_t key, double val,
                                int64_t from, int64_t to, int64_t m, int64_t* out, hipStream_t stream) {
    const size_t lds_bytes = (size_t)SMALL_W * (sizeof(int64_t) + sizeof(double));
    static PerDeviceOnce once;
    {
        hipError_t e = once.run([] {
            return hipFuncSetAttribute(reinterpret_cast<const void*>(k_dbg_raw), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        });
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_dbg_raw, dim3(1), dim3(SEQ_BLOCK), lds_bytes, stream, keys, vals, occ, sems, len, op, key, val, from, to, m, out);
    return hipGetLastError();
}

}  // namespace dsa
