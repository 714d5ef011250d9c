// csrc/parbatch.hip — batch-parallel writes for a vector's PMA: plan / resolve / apply.
//
// A batch is DEFINED as the reference's setindex! applied in order (src/pma.jl:196-213).  Two writes commute when the
// slots one of them reads to take its decisions or modifies are untouched by the other.  Per round, for the next G ops:
//
//   k_plan    (one wave per op, read-only): K-find (wave-parallel form), the shift target (_nextemptypos /
//             _previousemptypos, src/utils.jl:3-28) and the density-threshold scan of src/pma.jl:105-141 evaluated on the
//             PRE-round state, corrected by the op's own occupancy change.  The result is a Plan with the op's FOOTPRINT:
//             the hull of { predecessor slot and the slot after it (what find depends on), the shifted run, the accepted
//             window (every window whose count was consulted lies inside it) }.  Ops whose scan is not accepted within
//             PB_MAX_W slots (big rebalance, _extend!, _shrink!), or that are not vector writes, are BARRIERs.
//   resolve   (the workgroup of k_plan that finishes last, found by a ticket — no launch of its own): d = min(first BARRIER,
//             smallest j whose footprint overlaps the footprint of an EARLIER op).  Ops [0, d) are pairwise disjoint: each of
//             them sees, when executed alone in order, exactly the state it was planned on.  pb_resolve.h: one function per
//             stage, on one LDS state.
//   k_apply  (one wave per op): shift, write, occupancy update (atomics: footprints are disjoint in slots, not in 64-slot
//             bitmap words), then the small-window pack + spread through the wave's LDS slice.
//
// The host (writes_host.hip) applies the prefix in parallel and hands the op at d (and a growing chunk after it when the
// prefixes stay short, e.g. ascending appends) to the sequential sequencer.  Result: bit-identical to the sequential order.
//
// This file is the only translation unit; it includes two headers of its own.  pb_fpcheck.h: the footprint-check build
// (-DDSA_FP_CHECK) — recorders, check kernels, and the fp_* hooks the kernels here call (empty in the default build).
// pb_resolve.h: the resolve step.
#include "wave_dev.h"
#include "find_dev.h"

namespace dsa {
constexpr int PB_BLOCK = 256;                // k_apply: 4 waves = 4 ops per workgroup (32 KB of LDS per wave)
constexpr int PL_BLOCK = 1024;                // k_plan: 16 waves = 16 ops per workgroup; the workgroup that finishes last resolves the round with
                                              // one thread per op (with 256 threads the chain walks of the resolve step were the longest part of a round)
constexpr int PB_MAX_W_LOG2 = 11;
constexpr int PB_MAX_W = 1 << PB_MAX_W_LOG2;  // largest window a single wave rebalances (32 KB of LDS per wave, 128 KB per workgroup)
constexpr int PB_GMAX = ROUND_GMAX;           // ops planned per round at most (one wave each)

enum : int32_t { PB_NOOP = 0, PB_OVERWRITE = 1, PB_INS_R = 2, PB_INS_L = 3, PB_DELETE = 4, PB_BARRIER = 5, PB_NEWCOL = 6,
                 PB_DEFER = 7 /* written by the resolve step over the action of an op it defers: k_apply skips it */ };
constexpr int64_t PB_PEND_MAX = TABLE_PEND_MAX;  // the sequencer imports, tables.hip merges the pending table entries
constexpr size_t PB_WAVE_LDS = (size_t)PB_MAX_W * (sizeof(int64_t) + sizeof(double));      // dynamic LDS of one applying wave: the keys and values of its window

// an op whose density scan stopped at its leaf: nothing but the leaf's COUNT ties it to the rest of the leaf (Plan::lo / hi then hold
// the tight hull, see pb_plan_one)
__device__ __forceinline__ bool pb_is_leaf_only(int32_t action, int64_t ws, int64_t we, int64_t seg, int32_t count) {
    if (action == PB_NEWCOL) return (count & 0x80) != 0;
    return (action == PB_INS_R || action == PB_INS_L || action == PB_DELETE) && we - ws + 1 == seg;
}
// slot whose occupancy the op changes, and by how much
__device__ __forceinline__ int64_t pb_changed_slot(int32_t action, int64_t pos, int64_t aux) { return action == PB_DELETE ? pos : aux; }
// (a new column accepted by its leaf fills two gaps — Plan::aux and the end of its tight hull; one whose footprint is its window counts
// for nobody: no leaf-only op can share that window)
__device__ __forceinline__ int pb_delta(int32_t action, bool leaf_only = false) {
    return (action == PB_INS_R || action == PB_INS_L) ? 1 : (action == PB_DELETE ? -1 : ((action == PB_NEWCOL && leaf_only) ? 1 : 0));
}
// the FULL footprint of a plan where nobody keeps count per leaf (the local rounds): a leaf-only op is widened from its tight hull to its
// window; a new column without a fallback window (level 0x7f) has none to be widened to and takes the whole array
__device__ __forceinline__ void pb_full_footprint(const Plan& q, int64_t seg, int64_t capacity, int64_t& lo, int64_t& hi) {
    lo = q.lo; hi = q.hi;
    if (lo <= hi && pb_is_leaf_only(q.action, q.ws, q.we, seg, q.count)) {
        if (q.action == PB_NEWCOL && (q.count & 0x7f) == 0x7f) { lo = 1; hi = capacity; }
        else { if (q.ws < lo) lo = q.ws; if (q.we > hi) hi = q.we; }
    }
}
}  // namespace dsa

#include "pb_fpcheck.h"      // fp_*: the hooks of the footprint-check build (empty in the default build)

namespace dsa {
__device__ __forceinline__ uint64_t pb_occ_load(const uint64_t* occ, int64_t w) {
    // L2-served load: other waves of the same launch update neighbouring bits of shared words with device-scope atomics
    return __hip_atomic_load(occ + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// occupied cells of [ws, we] (1-based, inclusive), whole wave
__device__ int64_t pb_wave_count(const uint64_t* occ, int64_t ws, int64_t we, bool coherent) {
    const int64_t lo0 = ws - 1, hi0 = we - 1, w0 = lo0 >> 6, w1 = hi0 >> 6;
    int64_t c = 0;
    for (int64_t w = w0 + lane_id(); w <= w1; w += 64)
        c += popc64((coherent ? pb_occ_load(occ, w) : occ[w]) & word_range_mask(w, lo0, hi0));
    return wave_reduce_add(c);
}

// Plan of ONE op by one wave (read-only): what the op would do on the current state, and its footprint.  w = index of the op in its
// round (new columns take table entries in that order), max_w = largest window one wave of the caller rebalances.
__device__ Plan pb_plan_one(KeyArr keys, const double* vals, const uint64_t* occ, const int64_t* sems, const int64_t* col_keys,
                            const uint8_t* col_live, const Ctl* ctl, const Op op, int w, int max_w) {
    const int64_t capacity = ctl->capacity, seg = ctl->segment_capacity, height = ctl->height;
    Plan pl;
    pl.lo = 1; pl.hi = 0; pl.pos = 0; pl.aux = 0; pl.ws = 0; pl.we = 0; pl.count = 0; pl.action = PB_BARRIER;
    fp_reset();
    int why = 0;           // dev: reason of a BARRIER (kept in pl.count): 0 not plannable, 1 new column w/o successor or v == 0, 2 limits, 3 shifts, 4 sem leaf, 5 window, 6 scan
    // search range of the write: the whole array for a vector (src/pma.jl:196-213); for setindex!(mpcsc, v, row, col) on an
    // EXISTING live column, semaphore+1 .. end of partition for the insert path and semaphore .. end for the delete path
    // (src/pcsr.jl:294-310).  Anything else (new column, deleted partition, delete of a key <= 0 whose bisection is
    // path-dependent) is left to the sequential sequencer.
    bool plannable = false;
    int64_t from = 1, to = capacity, del_from = 1;
    if (op.kind == OP_VEC_SET) {
        plannable = true;
    } else if (op.kind == OP_MPCSC_SET && sems != nullptr && col_keys != nullptr) {
        const int64_t table_len = ctl->table_len, npend = ctl->n_pending, ns = table_len - npend;
        const bool dense = ctl->nb_partitions == table_len;          // no tombstone (always true while entries are pending)
        const DFoundKey tf = d_find_table_fast(col_keys, col_live, ns, op.b, dense);
        bool found = tf.has && tf.key == op.b;
        int64_t part = tf.pos;                                       // 1-based partition id
        // successor of op.b in key order (0-based table index, -1: none): first sorted entry with a larger key ...
        int64_t sidx = -1, skey = 0;
        if (dense) {
            const int64_t sorted_succ = tf.has ? tf.pos : 0;         // found: the next entry ; not found: #keys below
            if (sorted_succ < ns) { sidx = sorted_succ; skey = col_keys[sorted_succ]; }
            // ... or a pending entry (created by earlier rounds at the end of the tables, arrival order): wave-wide scan
            if (npend > 0) {
                int64_t bk = INT64_MAX, bi = -1, hit = -1;
                for (int64_t j = lane_id(); j < npend; j += 64) {
                    const int64_t k = col_keys[ns + j];
                    if (k == op.b) hit = ns + j;
                    if (k > op.b && k < bk) { bk = k; bi = ns + j; }
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    const int64_t k2 = __shfl_xor(bk, o, 64), i2 = __shfl_xor(bi, o, 64), h2 = __shfl_xor(hit, o, 64);
                    if (k2 < bk) { bk = k2; bi = i2; }
                    if (h2 > hit) hit = h2;
                }
                if (!found && hit >= 0) { found = true; part = hit + 1; }
                if (bi >= 0 && (sidx < 0 || bk < skey)) { sidx = bi; skey = bk; }
            }
        }
        if (found) {
            const int64_t sp = sems[part - 1];
            if (sp != 0 && (op.v != 0.0 || op.a > SEM_KEY)) {
                from = sp + 1; del_from = sp;
                if (dense) to = sidx >= 0 ? sems[sidx] - 1 : capacity;
                else {
                    const int64_t nxt = d_next_live_sem(sems, part, table_len);
                    to = nxt != 0 ? sems[nxt - 1] - 1 : capacity;
                }
                plannable = true;
            }
        } else if (!(dense && sidx >= 0 && op.v != 0.0)) { why = 1;
        } else if (!(npend + w + 1 <= PB_PEND_MAX && table_len + w + 1 <= ctl->table_cap)) { why = 2;
        } else {
            // NEW column in front of an existing one (addcolumn! + addpartition!(pcsc, prev), src/pcsr.jl:114-169, then the write):
            // its semaphore cell goes right in front of the successor's semaphore, the element right behind it — two
            // dependent inserts, each with its own density scan and possibly its own rebalance.  k_apply EXECUTES them in
            // order on the live state; the plan only proves that everything they can touch lies in one aligned window
            // [A, B] of level H (the footprint): both inserts shift to the right inside it, and the level-H window accepts
            // the count after one and after two new cells, so either scan stops at a level <= H, and the semaphore is not on
            // the window's last slot.  Then the element's insert stays inside too: the successor's semaphore follows the new
            // one in [A, B], so after a rebalance of a window W1 that holds both it is not the last cell of W1 and spread!
            // (src/moves.jl:120-140, last gap on one of the last two slots) leaves a gap behind it; if W1 ends ON the new
            // semaphore, or nothing was rebalanced, the second empty slot of the pre-round state (ne2 <= B) is still free.
            const int64_t p1 = sems[sidx] - 1;                        // _insert! after p1: the new semaphore lands on p1 + 1
            const int64_t ip1 = p1 + 1;
            const int64_t ne1 = d_next_empty(occ, p1, capacity);
            const int64_t ne2 = ne1 != 0 ? d_next_empty(occ, ne1, capacity) : 0;
            fp_pos(p1 + 1, ne2 != 0 ? ne2 : capacity);
            why = 3;
            if (p1 >= 1 && ne1 != 0 && ne2 != 0) {
                why = 5;
                // the fallback window: the first level H whose aligned window holds both gaps and accepts the count after one and after two new cells
                int64_t H = -1, A = 0, B = 0, cnt = 0;
                for (int64_t h = 0; h <= height; ++h) {
                    const int64_t W = seg << h;
                    if (W > max_w) break;
                    A = ((ip1 - 1) / W) * W + 1; B = A + W - 1;
                    if (ne2 > B || ip1 >= B) continue;
                    cnt = pb_wave_count(occ, A, B, false);
                    fp_cnt(A, B);
                    if (ctl->lo[h] <= cnt + 1 && cnt + 2 <= ctl->hi[h]) { H = h; break; }
                }
                // No window of a wave's size accepts (a small, fast-growing array sits between the thresholds of its middle levels and
                // the leaf's — config 5's first batches: 283 such new rows, each a detour through the sequencer although its leaf accepted and
                // nothing was rebalanced): the op can still be planned when its LEAF accepts — level 0x7f = "no fallback": the resolve step
                // cuts the prefix in front of it instead of widening it.
                {
                    const int32_t lvl = H >= 0 ? (int32_t)H : 0x7f;
                    if (H >= 0) {
                        pl.action = PB_NEWCOL; pl.pos = p1; pl.aux = ne1;
                        pl.ws = A; pl.we = B; pl.count = lvl | ((int32_t)cnt << 8);      // level, and the cells of [A, B] before the round
                        pl.lo = p1 < A ? p1 : A; pl.hi = B;
                    }
                    // Both scans accepted by the LEAF of the new semaphore (the element lands in the same leaf): neither insert is
                    // followed by a rebalance, the two shifted runs [p1 + 1, ne1] and [p1 + 2, ne2] are all that moves — wherever
                    // the two gaps are inside [A, B] (a run that leaves the leaf pushes one cell out for the one that comes in).
                    // The plan then carries that TIGHT hull, flag 0x80 and the leaf's cell count; the resolve step widens it to
                    // [A, B] unless the leaf accepts every order of the window's ops that change its count (pb_is_leaf_only).
                    const int64_t l0 = ((ip1 - 1) / seg) * seg + 1, l1 = l0 + seg - 1;
                    bool tight = false;
                    int32_t tcount = 0;
                    if (seg > 64) {
                        // (counts travel in 7 bits)
                    } else if (ip1 < l1) {
                        const int64_t cl = H == 0 ? cnt : pb_wave_count(occ, l0, l1, false);
                        fp_cnt(l0, l1);
                        const int64_t c1 = cl + (ne1 <= l1 ? 1 : 0), c2 = c1 + (ne2 <= l1 ? 1 : 0);
                        if (ctl->lo[0] <= c1 && c2 <= ctl->hi[0]) { tight = true; tcount = lvl | 0x80 | ((int32_t)cl << 8); }
                    } else if (l1 + seg <= capacity) {
                        // The semaphore lands on the LAST slot of its leaf (the successor's semaphore moves on into the next one), the
                        // element on the first slot of the next leaf: the first scan reads this leaf — its count unchanged —, the
                        // second the next one, which receives whatever gaps of its own the two runs fill.  Two leaves to accept
                        // (flag 0x8000 + the second count); without this a semaphore on slot 512 k needed a window of 1024 slots.
                        const int64_t m1 = l1 + seg;
                        const int64_t cl = pb_wave_count(occ, l0, l1, false), cm = pb_wave_count(occ, l1 + 1, m1, false);
                        fp_cnt(l0, l1); fp_cnt(l1 + 1, m1);
                        const int64_t c2 = cm + (ne1 <= m1 ? 1 : 0) + (ne2 <= m1 ? 1 : 0);
                        if (ctl->lo[0] <= cl && cl <= ctl->hi[0] && ctl->lo[0] <= cm && c2 <= ctl->hi[0]) {
                            tight = true; tcount = lvl | 0x80 | ((int32_t)cl << 8) | 0x8000 | ((int32_t)cm << 16);
                        }
                    }
                    if (tight) {
                        pl.action = PB_NEWCOL; pl.pos = p1; pl.aux = ne1;
                        pl.lo = p1; pl.hi = ne2; pl.count = tcount;
                    }
                }
            }
        }
    }
    if (plannable) {
        const DFound f = op.v != 0.0 ? d_find_fast(keys, vals, occ, op.a, from, to) : d_find_fast(keys, vals, occ, op.a, del_from, to);
        const bool exists = op.v != 0.0 ? (f.has && f.key == op.a && from <= f.pos && f.pos <= to)      // src/writes.jl:16
                                        : (f.has && f.key == op.a);                                     // src/writes.jl:59
        int64_t ip = 0, changed = 0, delta = 0, wlo = 1, whi = 0, rlo = 1, rhi = 0;
        bool scan = false;
        if (op.v != 0.0) {
            if (exists) {                                   // overwrite  src/writes.jl:16-19
                pl.action = PB_OVERWRITE; pl.pos = f.pos; pl.lo = f.pos; pl.hi = f.pos;
            } else {
                const int64_t p = f.pos;
                const int64_t ne = d_next_empty(occ, p, capacity);
                fp_pos(p + 1, ne != 0 ? ne : capacity);
                rlo = p >= 1 ? p : 1; rhi = p + 1 <= capacity ? p + 1 : capacity;
                if (ne != 0) { pl.action = PB_INS_R; ip = p + 1; changed = ne; wlo = p + 1; whi = ne; pl.aux = ne; scan = true; }
                else {
                    const int64_t pe = d_prev_empty(occ, p);
                    fp_pos(pe != 0 ? pe : 1, p - 1);
                    // (the left branch is taken because NO slot behind p is free up to the end of the array: the plan has read all of them —
                    // an earlier delete anywhere behind p would have sent this insert to the right instead.  Rounds 2-4 kept rhi = p + 1: an
                    // insert near the end of a full tail and a delete of the last cell ran in one round, tools/fuzz.py run_same_leaf seed 2000.)
                    if (pe != 0) { pl.action = PB_INS_L; ip = p; changed = pe; wlo = pe; whi = p; pl.aux = pe; scan = true; rhi = DSA_FP_REGRESS == 2 ? rhi : capacity; }
                }
                pl.pos = p; delta = 1;
            }
        } else {
            if (!exists) {                                  // delete of a missing key: nothing happens, but only as long as
                const int64_t p = f.pos;                    // nobody inserts that key first -> depends on slots p, p+1
                pl.action = PB_NOOP;
                pl.lo = p >= 1 ? p : 1; pl.hi = p + 1 <= capacity ? p + 1 : capacity;
            } else {
                pl.action = PB_DELETE; pl.pos = f.pos; ip = f.pos; changed = f.pos; delta = -1;
                wlo = whi = f.pos; rlo = rhi = f.pos; scan = true;
            }
        }
        if (scan) {
            bool accepted = false;
            int64_t ws = 1, we = 0, c = 0;
            for (int64_t h = 0; h <= height; ++h) {
                const int64_t W = seg << h;
                if (W > max_w && h > 0) break;
                ws = ((ip - 1) / W) * W + 1;
                we = ws + W - 1;
                c = pb_wave_count(occ, ws, we, false) + ((changed >= ws && changed <= we) ? delta : 0);
                fp_cnt(ws, we);
                if (ctl->lo[h] <= c && c <= ctl->hi[h]) { accepted = true; break; }
            }
            if (!accepted) {
                pl.action = PB_BARRIER; why = 6;
            } else {
                pl.ws = ws; pl.we = we; pl.count = (int32_t)c;
                // what the op reads for its decisions or moves, apart from the COUNT of its window: predecessor and the slot behind
                // it, the shifted run up to the gap it fills
                int64_t lo = wlo < rlo ? wlo : rlo, hi = whi > rhi ? whi : rhi;
                // accepted by its leaf (no rebalance follows): the plan carries this TIGHT hull; the resolve step widens it to the
                // leaf unless the leaf provably accepts every order of the window's ops that change its count (pb_is_leaf_only)
                if (we - ws + 1 != seg) { if (ws < lo) lo = ws; if (we > hi) hi = we; }
                pl.lo = lo; pl.hi = hi;
            }
        }
    }
    if (pl.action == PB_BARRIER) pl.count = why;
    return pl;
}
}  // namespace dsa

#include "pb_resolve.h"      // Round, Cells, Resolve and the resolve_* stages

namespace dsa {
// One wave per op plans it and publishes the plan; the workgroup that finishes last (a ticket; no second and third launch per round)
// resolves the round: the stages of pb_resolve.h in order, on one LDS state.  The __syncthreads() between two stage calls is the barrier
// that separates those stages; tk0 .. tr3 are the stage boundaries the dev profile (-DDSA_PB_PROF) sums cycles between.
__global__ __launch_bounds__(PL_BLOCK) void k_plan(const DevBufs* bufs, const Ctl* ctl, const Op* ops, RoundState* rs, Plan* plans) {
    // the round's window of ops comes from the device-resident cursor: rounds are enqueued back to back without host syncs
    const long long tk0 = clock64();
    if (rs->stop) return;
    const DevBufs db = *bufs;
    const KeyArr keys{db.keys, db.wide, 0};
    const Round R = pb_round_load(db, ctl, rs);                        // what the resolve step needs is requested NOW, in front of the plan (see Round)
    const int G = R.G;
    const int w = blockIdx.x * (PL_BLOCK / 64) + (threadIdx.x >> 6);
    if (w < G) {
        const Plan pl = pb_plan_one(keys, db.vals, db.occ, db.sems, db.col_keys, db.col_live, ctl, ops[R.op_index(w)], w, PB_MAX_W);
        // device-scope (write-through) stores: the workgroup that resolves the round may sit on another XCD; a release FENCE per
        // workgroup instead would write back that XCD's L2 (measured slower).  Seven lanes store one 8-byte field each: ONE store
        // instruction for the 56-byte plan instead of eight by lane 0.
        static_assert(sizeof(Plan) == 56, "the plan is published as seven 8-byte words");
        const int l = lane_id();
        if (l < 7) {
            const int64_t v = l == 0 ? pl.lo : l == 1 ? pl.hi : l == 2 ? pl.pos : l == 3 ? pl.aux : l == 4 ? pl.ws : l == 5 ? pl.we
                              : (int64_t)((uint64_t)(uint32_t)pl.count | ((uint64_t)(uint32_t)pl.action << 32));
            __hip_atomic_store(reinterpret_cast<int64_t*>(plans + w) + l, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        fp_publish_plan(plans, w);
    }
    // ---- the ticket ------------------------------------------------------------------------------------------------------------------
    __shared__ Resolve S;
    __builtin_amdgcn_s_waitcnt(0);                                     // the plan stores of this wave have been acknowledged at device scope
    const long long tk1 = clock64();
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned t = __hip_atomic_fetch_add(&rs->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        S.sLast = t == gridDim.x - 1 ? 1 : 0;
        S.sC = G; S.sB = G; S.sSumDn = 0; S.sSumRebN = 0; S.sSumRebW = 0u;
    }
    __syncthreads();
    if (!S.sLast) return;
    // ---- resolve, by the workgroup that finishes last --------------------------------------------------------------------------------
    const long long tr0 = clock64();
    const Cells hc = pb_cells(R.cap0, R.seg0);
    resolve_load(S, R, hc, ctl, plans);
    __syncthreads();
    const long long tr1 = clock64();
    const int Gc = S.sB < G ? S.sB : G;                                // ops at or behind the first BARRIER do not matter
    resolve_chain(S, hc, Gc);
    __syncthreads();
    resolve_leaf_counts(S, R, hc, Gc, rs);
    __syncthreads();
    resolve_overlaps(S, R, hc, Gc);
    __syncthreads();
    const long long tr2 = clock64();
    resolve_seal(S, R, hc, Gc, ctl, db.occ, rs);                       // (ends with its own barrier wherever it wrote)
    const long long tr3 = clock64();
    fp_publish_footprints(plans, S.sIv, Gc);
    const Verdict V = resolve_decide(S, R);
    const NextWindow N = resolve_next_window(S, R, V, const_cast<PendOp*>(db.pend) + (size_t)(1 - R.cur) * PB_GMAX);
    if (threadIdx.x == 0) { const long long t[6] = {tk0, tk1, tr0, tr1, tr2, tr3}; pbprof_round(S, R, V, plans, t); }
    resolve_commit(S, R, V, N, ctl, rs, plans);
}

// ---- apply ----------------------------------------------------------------------------------------------------------
// cells [a, b-1] -> +dist (_moverightloop!  src/moves.jl:32-36), highest chunk first: a chunk's stores land above every cell that is still
// to be read.  LIVE: the cells were just written by this wave (L2-served loads, see pb_next_empty_live).
template <bool LIVE>
__device__ void pb_shift_right(KeyArr keys, double* vals, int64_t* sems, int64_t a, int64_t b, int dist = 1) {
    const int lane = lane_id();
    fp_touch(a, b - 1 + dist);
    for (int64_t hi = b - 1; hi >= a; hi -= 64) {
        const int64_t p = hi - lane;
        const bool act = p >= a;
        int64_t k = 0; double v = 0.0;
        if (act) {
            k = LIVE ? keys.ld_agent(p - 1) : keys.ld(p - 1);
            v = LIVE ? __hip_atomic_load(vals + p - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : vals[p - 1];
        }
        if (act) {
            keys[p - 1 + dist] = k; vals[p - 1 + dist] = v;
            if (sems != nullptr && k == SEM_KEY) sems[(int64_t)v - 1] = p + dist;
        }
    }
}
__device__ void pb_shift_left(KeyArr keys, double* vals, int64_t* sems, int64_t a, int64_t b, bool last_occ) {   // cells [a+1, b] -> -1
    const int lane = lane_id();
    fp_touch(a, b);
    for (int64_t lo = a + 1; lo <= b; lo += 64) {
        const int64_t p = lo + lane;
        const bool act = p <= b && (p < b || last_occ);
        int64_t k = 0; double v = 0.0;
        if (act) { k = keys[p - 1]; v = vals[p - 1]; }
        if (act) {
            keys[p - 2] = k; vals[p - 2] = v;
            if (sems != nullptr && k == SEM_KEY) sems[(int64_t)v - 1] = p - 1;       // _moveleftloop!  src/moves.jl:75-79
        }
    }
}
__device__ __forceinline__ void pb_bit_set(uint64_t* occ, int64_t pos) {
    fp_touch(pos, pos);
    atomicOr((unsigned long long*)(occ + ((pos - 1) >> 6)), 1ull << ((pos - 1) & 63));
}
__device__ __forceinline__ void pb_bit_clear(uint64_t* occ, int64_t pos) {
    fp_touch(pos, pos);
    atomicAnd((unsigned long long*)(occ + ((pos - 1) >> 6)), ~(1ull << ((pos - 1) & 63)));
}

// pack! + spread! of [ws, we] (W <= PB_MAX_W) holding m cells, by one wave  (src/moves.jl:94-140)
__device__ void pb_wave_rebalance(KeyArr keys, double* vals, uint64_t* occ, int64_t* sems, int64_t ws, int64_t we, int64_t m,
                                  int64_t* sK, double* sV) {
    const int lane = lane_id();
    const int64_t W = we - ws + 1, lo0 = ws - 1, w0 = lo0 >> 6;
    const SpreadGeom g = make_geom(W, m);
    fp_touch(ws, we);
    if (W >= 64) {
        const int nwords = (int)(W >> 6);                          // <= 16
        const uint64_t myword = lane < nwords ? pb_occ_load(occ, w0 + lane) : 0ull;
        const uint32_t myoff = wave_excl_scan((uint32_t)popc64(myword));
        for (int w = 0; w < nwords; ++w) {
            const uint64_t mask = __shfl(myword, w, 64);
            const uint32_t off = __shfl(myoff, w, 64);
            if ((mask >> lane) & 1ull) {
                const uint32_t r = off + (uint32_t)popc64(mask & mask_lt(lane));
                const int64_t s = ((w0 + w) << 6) + lane;
                // L2-served loads: some of these cells were just written by this wave's own shift
                sK[r] = keys.ld_agent(s);
                sV[r] = __hip_atomic_load(vals + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_s_waitcnt(0xc07f);                        // lgkmcnt(0): the wave's LDS writes have landed
        for (int64_t base = 0; base < W; base += 64) {
            const int q = (int)base + lane + 1;
            bool occd = false;
            int rank;
            if (!slot_is_gap(g, q, &rank)) {
                occd = true;
                const int64_t k = sK[rank - 1];
                const double v = sV[rank - 1];
                keys[lo0 + q - 1] = k;
                vals[lo0 + q - 1] = v;
                if (sems != nullptr && k == SEM_KEY) sems[(int64_t)v - 1] = lo0 + q;       // spread! with semaphores  src/moves.jl:160-166
            }
            const uint64_t b = __ballot(occd);
            if (lane == 0) __hip_atomic_store(occ + w0 + (base >> 6), b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    } else {
        const int bit0 = (int)(lo0 & 63);
        const uint64_t wmask = ((1ull << W) - 1ull) << bit0;
        const uint64_t word = pb_occ_load(occ, w0);
        const uint64_t mask = (word & wmask) >> bit0;
        if (lane < W && ((mask >> lane) & 1ull)) {
            const int r = popc64(mask & mask_lt(lane));
            sK[r] = keys.ld_agent(lo0 + lane);
            sV[r] = __hip_atomic_load(vals + lo0 + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_s_waitcnt(0xc07f);
        bool occd = false;
        const int q = lane + 1;
        if (q <= W) {
            int rank;
            if (!slot_is_gap(g, q, &rank)) {
                occd = true;
                const int64_t k = sK[rank - 1];
                const double v = sV[rank - 1];
                keys[lo0 + q - 1] = k;
                vals[lo0 + q - 1] = v;
                if (sems != nullptr && k == SEM_KEY) sems[(int64_t)v - 1] = lo0 + q;
            }
        }
        const uint64_t b = __ballot(occd);
        if (lane == 0) {                                           // only this op's bits of the shared word change
            atomicAnd((unsigned long long*)(occ + w0), ~wmask);
            atomicOr((unsigned long long*)(occ + w0), (b << bit0) & wmask);
        }
    }
}

// ---- pieces of k_apply that run on the LIVE state of the op's footprint (cells and bits this wave has just written):
// L2-served loads, after the wave's own stores have been acknowledged
__device__ int64_t pb_next_empty_live(const uint64_t* occ, int64_t from, int64_t capacity) {          // _nextemptypos  src/utils.jl:3-10
    if (from + 1 > capacity) return 0;
    int64_t w = from >> 6;
    uint64_t word = ~pb_occ_load(occ, w) & ~mask_lt((int)(from & 63));
    const int64_t lastw = (capacity - 1) >> 6;
    while (true) {
        if (word) { const int64_t p = (w << 6) + __ffsll((unsigned long long)word); fp_touch(from + 1, p <= capacity ? p : capacity); return p <= capacity ? p : 0; }
        if (++w > lastw) { fp_touch(from + 1, capacity); return 0; }
        word = ~pb_occ_load(occ, w);
    }
}
// _look_for_rebalance! + _even_rebalance! (src/pma.jl:94-141) around `ip` on the live bitmap; the plan guarantees acceptance
// at a level whose window fits one wave.  Returns true when cells were moved.
__device__ bool pb_scan_and_rebalance_live(KeyArr keys, double* vals, uint64_t* occ, int64_t* sems, Ctl* ctl, int64_t ip, int64_t hmax,
                                           int64_t* sK, double* sV) {
    const int64_t seg = ctl->segment_capacity;
    int64_t ws = 1, we = 0, c = 0, W = seg;
    for (int64_t h = 0; h <= hmax; ++h) {
        W = seg << h;
        ws = ((ip - 1) / W) * W + 1;
        we = ws + W - 1;
        c = pb_wave_count(occ, ws, we, true);
        if (ctl->lo[h] <= c && c <= ctl->hi[h]) break;
    }
    if (W == seg) return false;
    pb_wave_rebalance(keys, vals, occ, sems, ws, we, c, sK, sV);
    if (lane_id() == 0) {
        atomicAdd((unsigned long long*)&ctl->stat_rebalances, 1ull);
        atomicAdd((unsigned long long*)&ctl->stat_window_slots, (unsigned long long)W);
        atomicAdd((unsigned long long*)&ctl->stat_small_rebalances, 1ull);
    }
    return true;
}

// ONE planned op applied by one wave: shift, write, occupancy update, then the small-window pack + spread through the wave's LDS slice
// (sK / sV).  fault: raised if an op leaves its planned footprint (cannot happen, checked by the host).
// counted: the caller has already added the element delta of inserts / deletes and the statistics of their rebalances to the control
// block (k_plan's resolve step, once per round: one atomic per op on the same three or four words cost 4 us per round of ~500 ops).
__device__ void pb_apply_one(KeyArr keys, double* vals, uint64_t* occ, int64_t* sems, int64_t* col_keys, uint8_t* col_live, Ctl* ctl,
                             int32_t* fault, const Op op, const Plan pl, int64_t* sK, double* sV, const bool counted) {
    const int lane = lane_id();
    const int64_t seg = ctl->segment_capacity;
    int64_t delta = 0;
    fp_reset();
    switch (pl.action) {
        case PB_OVERWRITE:
            fp_touch(pl.pos, pl.pos);
            if (lane == 0) vals[pl.pos - 1] = op.v;
            break;
        case PB_INS_R: {                                           // _insert!, right branch  src/writes.jl:29-32
            const int64_t p = pl.pos, ne = pl.aux;
            pb_shift_right<false>(keys, vals, sems, p + 1, ne);
            if (lane == 0) { keys[p] = op.a; vals[p] = op.v; pb_bit_set(occ, ne); }
            delta = 1;
            break;
        }
        case PB_INS_L: {                                           // _insert!, left branch  src/writes.jl:34-37
            const int64_t p = pl.pos, pe = pl.aux;
            const bool last_occ = (pb_occ_load(occ, (p - 1) >> 6) >> ((p - 1) & 63)) & 1ull;
            pb_shift_left(keys, vals, sems, pe, p, last_occ);
            if (lane == 0) {
                keys[p - 1] = op.a; vals[p - 1] = op.v;
                if (pe < p - 1) { pb_bit_set(occ, pe); if (!last_occ) pb_bit_clear(occ, p - 1); }
                else if (last_occ) pb_bit_set(occ, pe);
                pb_bit_set(occ, p);
            }
            delta = 1;
            break;
        }
        case PB_DELETE:
            if (lane == 0) pb_bit_clear(occ, pl.pos);
            delta = -1;
            break;
        case PB_NEWCOL: {                                          // new column + its first element: two inserts in order (see k_plan)
            const int64_t p1 = pl.pos, ne1 = pl.aux, capacity = ctl->capacity;
            const int64_t hmax = (pl.count & 0x7f) <= ctl->height ? (pl.count & 0x7f) : ctl->height;      // (0x7f: leaf-accepted without a fallback window — both scans stop at the leaf)
            // (flag 0x80, tight hull: the leaf accepts both scans whatever the other ops of the round do to its count — the loop below stops at
            // level 0 on any count it can read; footprint widened by the resolve step: the window is this op's alone, the scan sees the planned state)
            const int64_t flo = pl.lo < pl.ws ? pl.lo : pl.ws, fhi = pl.hi > pl.we ? pl.hi : pl.we;
            // ids are labels: the next free table entry, whatever the key order (merged by the sequencer: Ctl::n_pending)
            int64_t idx = 0;
            if (lane == 0) {
                idx = (int64_t)atomicAdd((unsigned long long*)&ctl->table_len, 1ull);
                atomicAdd((unsigned long long*)&ctl->n_pending, 1ull);
                atomicAdd((unsigned long long*)&ctl->nb_partitions, 1ull);
                atomicAdd((unsigned long long*)&ctl->nb_elements, 2ull);
            }
            idx = __shfl(idx, 0, 64);
            // addpartition!: the semaphore cell (0, id) in front of the successor's semaphore  src/pcsr.jl:136-144
            pb_shift_right<false>(keys, vals, sems, p1 + 1, ne1);
            if (lane == 0) {
                keys[p1] = SEM_KEY; vals[p1] = (double)(idx + 1);
                sems[idx] = p1 + 1; col_keys[idx] = op.b; col_live[idx] = 1;
                pb_bit_set(occ, ne1);
            }
            __builtin_amdgcn_s_waitcnt(0);
            const bool moved = pb_scan_and_rebalance_live(keys, vals, occ, sems, ctl, p1 + 1, hmax, sK, sV);
            __builtin_amdgcn_s_waitcnt(0);
            const int64_t s1 = moved ? __hip_atomic_load(sems + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : p1 + 1;
            // setindex!(pcsc, value, key, partition) into the empty partition: find() returns the semaphore, insert behind it
            const int64_t ne2 = pb_next_empty_live(occ, s1, capacity);
            if (ne2 == 0 || ne2 > fhi || s1 < flo || s1 >= fhi) {
                // cannot happen (see k_plan); if it ever does, fail loudly instead of writing outside the footprint
                if (lane == 0) atomicExch(fault, 1);      // RoundState::pad = fault flag, read by the host after every burst
                break;
            }
            pb_shift_right<true>(keys, vals, sems, s1 + 1, ne2);
            if (lane == 0) { keys[s1] = op.a; vals[s1] = op.v; pb_bit_set(occ, ne2); }
            __builtin_amdgcn_s_waitcnt(0);
            pb_scan_and_rebalance_live(keys, vals, occ, sems, ctl, s1 + 1, hmax, sK, sV);
            break;
        }
        default:
            break;
    }
    if (delta != 0) {
        if (lane == 0 && !counted) atomicAdd((unsigned long long*)&ctl->nb_elements, (unsigned long long)delta);
        const int64_t W = pl.we - pl.ws + 1;
        if (W != seg) {                                            // _even_rebalance!  src/pma.jl:94-103
            __builtin_amdgcn_s_waitcnt(0);                         // the op's own stores / atomics are complete
            pb_wave_rebalance(keys, vals, occ, sems, pl.ws, pl.we, pl.count, sK, sV);
            if (lane == 0 && !counted) {
                atomicAdd((unsigned long long*)&ctl->stat_rebalances, 1ull);
                atomicAdd((unsigned long long*)&ctl->stat_window_slots, (unsigned long long)W);
                atomicAdd((unsigned long long*)&ctl->stat_small_rebalances, 1ull);
            }
        }
    }
}

__global__ __launch_bounds__(PB_BLOCK) void k_apply(const DevBufs* bufs, Ctl* ctl, const Op* ops, const RoundState* rs, const Plan* plans) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pb_lds[];
    if (rs->stop) return;
    const DevBufs db = *bufs;
    const KeyArr keys{db.keys, db.wide, 0};
    double* vals = db.vals; uint64_t* occ = db.occ;
    int64_t* sems = db.sems; int64_t* col_keys = db.col_keys; uint8_t* col_live = db.col_live;
    const int64_t i0 = rs->cursor;
    const int d = rs->d, np = rs->np;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int w = blockIdx.x * (PB_BLOCK / 64) + wv;
    if (w == 0 && lane == 0) const_cast<RoundState*>(rs)->G = rs->G_next;     // group size of the NEXT round (G is not read any more)
    if (w >= d) return;
    int64_t* sK = reinterpret_cast<int64_t*>(pb_lds) + (size_t)wv * PB_MAX_W;
    double* sV = reinterpret_cast<double*>(pb_lds + (size_t)(PB_BLOCK / 64) * PB_MAX_W * sizeof(int64_t)) + (size_t)wv * PB_MAX_W;
    // (plan and op are requested together: the op's address does not depend on the plan)
    const int64_t oi = w < np ? db.pend[(size_t)rs->cur * PB_GMAX + w].op : i0 + (w - np);
    const Op op = ops[oi];
    const Plan pl = plans[w];
    if (pl.action == PB_DEFER) return;                                          // deferred by the resolve step: pending for the next round
    if (fp_shadow_applied(rs)) return;                                          // (footprint-check build, mode 2: k_fp_pre has applied the prefix)
    pb_apply_one(keys, vals, occ, sems, col_keys, col_live, ctl, &const_cast<RoundState*>(rs)->pad, op, pl, sK, sV, true);
    fp_publish_touched(plans, w);
}

// ---- local rounds: the same plan / resolve / apply, by ONE workgroup, for phases with little parallelism --------------------------
// A grid round costs two launches (~15 us) whatever it applies; while the conflict-free prefixes are short — a small, fast-growing
// array whose windows are wide relative to it (the first batches of config 5: 19 ops per round), a small vector — the launches are
// all there is.  Here one persistent workgroup plans the next LR_WAVES ops (one wave each), decides the prefix in LDS, applies it,
// and goes on: a mini-round is two workgroup barriers instead of two launches.  Between mini-rounds the waves' stores are waited
// for and the scalar and vector L1 caches are invalidated (everything runs on one CU and one L2; the counters of the control block
// change by atomics at the L2).  The kernel leaves at an op that cannot be planned or after 16 one-op prefixes in a row (stop = 1: the
// sequencer), when the batch is done (2), when eight mini-rounds in a row applied all their ops (3: parallelism is back, grid
// rounds), or after max_rounds.
constexpr int LR_WAVES = 8;
constexpr int LR_MAX_W = 1024;                // largest window a wave rebalances here (16 KB of LDS per wave)
constexpr int LR_BLOCK = LR_WAVES * 64;

__global__ __launch_bounds__(LR_BLOCK) void k_local_rounds(const DevBufs* bufs, Ctl* ctl, const Op* ops, RoundState* rs, int max_rounds) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lr_lds[];
    __shared__ Plan sPlan[LR_WAVES];
    __shared__ int sD;
    const DevBufs db = *bufs;
    const KeyArr keys{db.keys, db.wide, 0};
    double* vals = db.vals; uint64_t* occ = db.occ;
    int64_t* sems = db.sems; int64_t* col_keys = db.col_keys; uint8_t* col_live = db.col_live;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int64_t* sK = reinterpret_cast<int64_t*>(lr_lds) + (size_t)wv * LR_MAX_W;
    double* sV = reinterpret_cast<double*>(lr_lds + (size_t)LR_WAVES * LR_MAX_W * sizeof(int64_t)) + (size_t)wv * LR_MAX_W;
    int64_t cursor = rs->cursor_n;                    // (the host drains the pending list of the grid rounds before it comes here: np_n == 0)
    const int64_t limit = rs->limit;
    int rounds = 0, stop = 0, why = 0, full_streak = 0, single_streak = 0;
    int64_t par_ops = 0;
    while (rounds < max_rounds) {
        const int64_t left = limit - cursor;
        if (left <= 0) { stop = 2; break; }
        const int G = (int)(left < LR_WAVES ? left : LR_WAVES);
        // ---- plan: one wave per op
        if (wv < G) {
            const Plan pl = pb_plan_one(keys, vals, occ, sems, col_keys, col_live, ctl, ops[cursor + wv], wv, LR_MAX_W);
            if (lane == 0) sPlan[wv] = pl;
        }
        __syncthreads();
        // ---- decide: d = min(first BARRIER, smallest j whose footprint overlaps the footprint of an earlier op)
        if (threadIdx.x == 0) {
            const int64_t seg = ctl->segment_capacity, capacity = ctl->capacity;
            int dd = G;
            for (int j = 0; j < G && dd == G; ++j) {
                if (sPlan[j].action == PB_BARRIER) { dd = j; break; }
                // (leaf-only ops carry their tight hull: widened to their window here — no count bookkeeping in the mini-rounds)
                int64_t lo, hi;
                pb_full_footprint(sPlan[j], seg, capacity, lo, hi);
                if (lo > hi) continue;
                for (int i = 0; i < j; ++i) {
                    int64_t l2, h2;
                    pb_full_footprint(sPlan[i], seg, capacity, l2, h2);
                    if (l2 <= h2 && l2 <= hi && lo <= h2) { dd = j; break; }
                }
            }
            sD = dd;
        }
        __syncthreads();
        const int dd = sD;
        if (dd == 0) { stop = 1; why = sPlan[0].count & 7; break; }       // the op at the cursor cannot be planned: the sequencer's
        // ---- apply: the prefix, one wave per op (footprint-check build: one op after the other in mode 2, records kept and checked in mode 1)
        if (!fp_lr_shadow(keys, vals, occ, sems, col_keys, col_live, ctl, ops, rs, sPlan, dd, cursor, LR_MAX_W, sK, sV)) {
            fp_lr_keep_plan_record(dd);
            if (wv < dd) pb_apply_one(keys, vals, occ, sems, col_keys, col_live, ctl, &rs->pad, ops[cursor + wv], sPlan[wv], sK, sV, false);
            fp_lr_check_sets<LR_WAVES>(rs, ctl, sPlan, dd);
        }
        // ---- advance
        cursor += dd; par_ops += dd; ++rounds;
        full_streak = dd == LR_WAVES ? full_streak + 1 : 0;
        single_streak = (dd == 1 && G > 1) ? single_streak + 1 : 0;
        __builtin_amdgcn_s_waitcnt(0);                 // this wave's stores and atomics have been acknowledged
        __syncthreads();
        __builtin_amdgcn_s_dcache_inv();               // what the next plans read through the scalar cache ...
        asm volatile("buffer_inv sc0" ::: "memory");          // ... and the vector L1 of this CU (not the L2: everything here runs on one XCD)
        if (full_streak >= 8) { stop = 3; break; }
        if (single_streak >= 16) { stop = 1; why = 7; break; }          // every op collides with its predecessor (appends, one hot key): the sequencer's
    }
    if (threadIdx.x == 0) {
        rs->cursor = cursor; rs->cursor_n = cursor; rs->d = 0; rs->pend0 = cursor;
        rs->rounds += rounds; rs->par_ops += par_ops;
        rs->stop = stop;
        if (stop == 1) rs->why[why] += 1;
    }
}

// The last kernel of a burst: the round state and the control block go straight into the host's pinned mirrors, then the burst number
// into the word the host polls (system-scope stores, a release in between).  Replaces two device-to-host copy commands and a stream
// synchronisation per burst (~300 us of rounds each).
__global__ __launch_bounds__(256) void k_publish(const RoundState* rs, const Ctl* ctl, BurstPublish pub) {
    static_assert(sizeof(RoundState) % 8 == 0 && sizeof(Ctl) % 8 == 0, "copied as 8-byte words");
    const unsigned long long* src_rs = reinterpret_cast<const unsigned long long*>(rs);
    const unsigned long long* src_ctl = reinterpret_cast<const unsigned long long*>(ctl);
    unsigned long long* dst_rs = reinterpret_cast<unsigned long long*>(pub.host_rs);
    unsigned long long* dst_ctl = reinterpret_cast<unsigned long long*>(pub.host_ctl);
    constexpr int NRS = (int)(sizeof(RoundState) / 8), NCTL = (int)(sizeof(Ctl) / 8);
    for (int i = threadIdx.x; i < NRS + NCTL; i += 256) {
        const unsigned long long v = i < NRS ? __hip_atomic_load(src_rs + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                             : __hip_atomic_load(src_ctl + (i - NRS), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(i < NRS ? dst_rs + i : dst_ctl + (i - NRS), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
    if (threadIdx.x == 0) {
        publish_seq(pub.host_seq, (unsigned long long)(unsigned int)rs->seq);
    }
}
static void enqueue_publish(const RoundState* rs, const Ctl* ctl, BurstPublish pub, hipStream_t stream) {
    if (pub.host_seq != nullptr) hipLaunchKernelGGL(k_publish, dim3(1), dim3(256), 0, stream, rs, ctl, pub);      // (no mirror: the caller reads the state itself)
}

hipError_t launch_local_rounds(const DevBufs* bufs, Ctl* ctl, const Op* ops, RoundState* rs, int max_rounds, BurstPublish pub, hipStream_t stream) {
    constexpr size_t lds = (size_t)LR_WAVES * LR_MAX_W * (sizeof(int64_t) + sizeof(double));
    static PerDeviceOnce once;
    hipError_t e = once.run([] {
        return hipFuncSetAttribute(reinterpret_cast<const void*>(k_local_rounds), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    });
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_local_rounds, dim3(1), dim3(LR_BLOCK), lds, stream, bufs, ctl, ops, rs, max_rounds);
    enqueue_publish(rs, ctl, pub, stream);
    return hipGetLastError();
}

// one round = plan (+ resolve and cursor advance by its last workgroup) -> apply, all driven by the device-resident RoundState
static hipError_t configure_apply() {
    static PerDeviceOnce once;
    return once.run([] {
        return hipFuncSetAttribute(reinterpret_cast<const void*>(k_apply), hipFuncAttributeMaxDynamicSharedMemorySize, (int)((PB_BLOCK / 64) * PB_WAVE_LDS));
    });
}
static hipError_t enqueue_round(const DevBufs* bufs, Ctl* ctl, const Op* ops, RoundState* rs, Plan* plans, hipStream_t stream) {
    hipLaunchKernelGGL(k_plan, dim3(PB_GMAX / (PL_BLOCK / 64)), dim3(PL_BLOCK), 0, stream, bufs, ctl, ops, rs, plans);
    fp_enqueue_pre(bufs, ctl, ops, rs, plans, stream);
    hipLaunchKernelGGL(k_apply, dim3(PB_GMAX / 4), dim3(PB_BLOCK), (PB_BLOCK / 64) * PB_WAVE_LDS, stream, bufs, ctl, ops, rs, plans);
    fp_enqueue_post(rs, plans, ctl, stream);
    return hipGetLastError();
}

// A burst of `rounds` rounds.  The launch sequence depends only on pointers, so it is captured once into a hipGraph and
// replayed (one graph launch instead of 2 x rounds kernel launches: the rounds are launch-bound); the slot buffers and tables
// are reached through DevBufs, so the graph only changes when a bigger batch re-allocates the op array.  Falls back to eager
// launches when the stream cannot be captured.
hipError_t launch_burst(const DevBufs* bufs, Ctl* ctl, const Op* ops, RoundState* rs, Plan* plans, int rounds, BurstGraph* cache,
                        BurstPublish pub, hipStream_t stream) {
    hipError_t e = configure_apply();
    if (e != hipSuccess) return e;
    const void* key[12] = {bufs, ctl, ops, rs, plans, (const void*)(intptr_t)rounds, pub.host_rs, pub.host_ctl, pub.host_seq, nullptr, nullptr, nullptr};
    bool same = cache->exec != nullptr && cache->stream == stream;
    for (int k = 0; k < 12 && same; ++k) same = cache->key[k] == key[k];
    if (cache->disabled && cache->failed_on != stream) cache->disabled = false;      // another stream: capture may work there
    if (!same && !cache->disabled) {
        if (cache->exec) { (void)hipGraphExecDestroy(cache->exec); cache->exec = nullptr; }
        if (cache->graph) { (void)hipGraphDestroy(cache->graph); cache->graph = nullptr; }
        if (hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal) == hipSuccess) {
            for (int r = 0; r < rounds; ++r) (void)enqueue_round(bufs, ctl, ops, rs, plans, stream);
            enqueue_publish(rs, ctl, pub, stream);
            hipGraph_t g = nullptr;
            e = hipStreamEndCapture(stream, &g);
            if (e == hipSuccess && g != nullptr && hipGraphInstantiate(&cache->exec, g, nullptr, nullptr, 0) == hipSuccess) {
                cache->graph = g;
                for (int k = 0; k < 12; ++k) cache->key[k] = key[k];
                cache->stream = stream;
            } else {
                if (g) (void)hipGraphDestroy(g);
                cache->exec = nullptr; cache->disabled = true; cache->failed_on = stream;
                (void)hipGetLastError();
            }
        } else {
            cache->disabled = true; cache->failed_on = stream;
            (void)hipGetLastError();
        }
    }
    if (cache->exec != nullptr && !cache->disabled) return hipGraphLaunch(cache->exec, stream);
    for (int r = 0; r < rounds; ++r) {
        e = enqueue_round(bufs, ctl, ops, rs, plans, stream);
        if (e != hipSuccess) return e;
    }
    enqueue_publish(rs, ctl, pub, stream);
    return hipGetLastError();
}

void burst_graph_destroy(BurstGraph* cache) {
    if (cache->exec) (void)hipGraphExecDestroy(cache->exec);
    if (cache->graph) (void)hipGraphDestroy(cache->graph);
    *cache = BurstGraph();
}

// ---- parity hooks (include/dsa.h: dsa_dbg_raw_*), wave-level engine ------------------------------------------------------------
// The primitives one WAVE of k_apply uses — pb_shift_right / pb_shift_left with the occupancy atomics of pb_apply_one, and
// pb_wave_rebalance — on a caller-supplied raw slot array (see k_dbg_raw in sequencer.hip for the workgroup-level engine and the
// layout of out[]).  One wave, one op.
__global__ __launch_bounds__(64) void k_dbg_raw_wave(KeyArr keys, double* vals, uint64_t* occ, int64_t* sems, int64_t len, int op,
                                                     int64_t key, double val, int64_t from, int64_t to, int64_t m, int64_t* out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pb_lds[];
    int64_t* sK = reinterpret_cast<int64_t*>(pb_lds);
    double* sV = reinterpret_cast<double*>(pb_lds + (size_t)PB_MAX_W * sizeof(int64_t));
    const int lane = lane_id();
    int64_t err = 0, r_pos = 0, r_flag = 0, r_key = 0; double r_val = 0.0;
    switch (op) {
        case DBG_FIND: case DBG_FIND_FAST: {
            const DFound f = op == DBG_FIND ? d_find(keys, vals, occ, key, from, to) : d_find_fast(keys, vals, occ, key, from, to);
            r_pos = f.pos; r_flag = f.has ? 1 : 0; r_key = f.key; r_val = f.val;
            break;
        }
        case DBG_INSERT: case DBG_INSERT_FAST: {                   // insert! + _insert!  src/writes.jl:14-43, the way k_plan / k_apply split it
            const DFound f = op == DBG_INSERT ? d_find(keys, vals, occ, key, from, to) : d_find_fast(keys, vals, occ, key, from, to);
            if (f.has && f.key == key && from <= f.pos && f.pos <= to) {
                if (lane == 0) vals[f.pos - 1] = val;              // PB_OVERWRITE
                r_pos = f.pos;
                break;
            }
            const int64_t p = f.pos;
            const int64_t ne = d_next_empty(occ, p, len);
            r_flag = 1;
            if (ne != 0) {                                         // PB_INS_R
                pb_shift_right<false>(keys, vals, sems, p + 1, ne);
                if (lane == 0) { keys[p] = key; vals[p] = val; pb_bit_set(occ, ne); }
                r_pos = p + 1;
                break;
            }
            const int64_t pe = d_prev_empty(occ, p);
            if (pe == 0) { err = E_FULL; break; }
            const bool last_occ = (pb_occ_load(occ, (p - 1) >> 6) >> ((p - 1) & 63)) & 1ull;     // PB_INS_L
            pb_shift_left(keys, vals, sems, pe, p, last_occ);
            if (lane == 0) {
                keys[p - 1] = key; vals[p - 1] = val;
                if (pe < p - 1) { pb_bit_set(occ, pe); if (!last_occ) pb_bit_clear(occ, p - 1); }
                else if (last_occ) pb_bit_set(occ, pe);
                pb_bit_set(occ, p);
            }
            r_pos = p;
            break;
        }
        case DBG_DELETE: case DBG_DELETE_FAST: {                   // PB_DELETE
            const DFound f = op == DBG_DELETE ? d_find(keys, vals, occ, key, from, to) : d_find_fast(keys, vals, occ, key, from, to);
            if (f.has && f.key == key) { if (lane == 0) pb_bit_clear(occ, f.pos); r_pos = f.pos; r_flag = 1; }
            break;
        }
        case DBG_REBALANCE:
            pb_wave_rebalance(keys, vals, occ, sems, from, to, m, sK, sV);
            break;
        default:
            err = E_ARG;
    }
    if (lane == 0) { out[0] = err; out[1] = r_pos; out[2] = r_flag; out[3] = r_key; out[4] = __double_as_longlong(r_val); out[5] = 0; }
}

hipError_t launch_dbg_raw_wave(KeyArr keys, double* vals, uint64_t* occ, int64_t* sems, int64_t len, int op, int64_t key, double val,
                               int64_t from, int64_t to, int64_t m, int64_t* out, hipStream_t stream) {
    hipLaunchKernelGGL(k_dbg_raw_wave, dim3(1), dim3(64), PB_WAVE_LDS, stream, keys, vals, occ, sems, len, op, key, val, from, to, m, out);
    return hipGetLastError();
}

}  // namespace dsa

#ifdef DSA_PB_PROF
extern "C" void dsa_dbg_pbprof_dump(void) {
    unsigned long long h[32] = {0};
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(dsa::g_pbprof), sizeof(h)) != hipSuccess) return;
    const double r = h[0] ? (double)h[0] : 1.0;
    fprintf(stderr, "pbprof: %llu resolves, G %.0f applied %.0f conflicts %.2f | cycles per round: entry->planned %.0f ->ticket %.0f | load %.0f conflicts %.0f seal %.0f decide+list %.0f\n",
            h[0], h[8] / r, h[9] / r, h[7] / r, h[1] / r, h[2] / r, h[3] / r, h[4] / r, h[5] / r, h[6] / r);
    fprintf(stderr, "        rounds ended by: whole window %llu | prefix rule (run-ahead off) %llu, first conflict in the last eighth %llu, > 96 conflicts %llu | sealing: > 64 ops in the zone %llu, "
            "not a plain write %llu, no level fits %llu, zones touch %llu, a later op straddles a zone %llu | new column without a window %llu | barrier op [unplannable %llu newcol %llu limits %llu shifts %llu "
            "semleaf %llu window %llu scan %llu other %llu]\n", h[12], h[13], h[14], h[15], h[16], h[17], h[18], h[19], h[20], h[21], h[23], h[24], h[25], h[26], h[27], h[28], h[29], h[30]);
    unsigned long long z[32] = {0};
    (void)hipMemcpyToSymbol(HIP_SYMBOL(dsa::g_pbprof), z, sizeof(z));
}
#endif
