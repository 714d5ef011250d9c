// csrc/pb_resolve.h — the resolve step of a round of the batch-parallel writes, run by the workgroup of k_plan that finishes last.
// Included by parbatch.hip alone, behind pb_plan_one.
//
// The step folds the previous round's prefix into the cursor and decides this round's prefix d = min(first BARRIER, smallest j whose
// footprint overlaps the footprint of an earlier op): ops [0, d) are pairwise disjoint, each sees exactly the state it was planned on.
// k_apply works on (cursor, d).  Under run-ahead an op that conflicts with an earlier one is deferred to the next round and sealed in a
// zone, and the ops behind it that stay clear of that zone are applied all the same.
//
// One LDS object (Resolve) holds what the stages hand to each other; the scalars of the round (Round) and the geometry of the spatial
// hash (Cells) travel by value.  k_plan calls the stages in this order:
//     load -> chain -> leaf counts -> overlaps -> seal -> decide -> next window -> commit
// A __syncthreads() that separates two stages stands between the two calls in k_plan, next to the profile timestamp of that boundary;
// the barriers inside a stage separate its own passes.  Each stage's header says what it reads and writes.
#pragma once

namespace dsa {
#ifdef DSA_PB_PROF
__device__ unsigned long long g_pbprof[32];
#define PBW(S_, j_, code_) ((S_).sCutWhy[(j_)] = (unsigned char)(code_))
#else
#define PBW(S_, j_, code_) ((void)0)
#endif

// ---- the scalars of a round ------------------------------------------------------------------------------------------------------------
// Filled at the top of k_plan by EVERY workgroup, in front of the plan: the workgroup that resolves the round does not start with a
// dependent round trip to memory (~2 us across XCDs), and the fields of the round state the step folds at its very end are scalar loads
// instead of dependent round trips of one thread behind the last barrier — nobody writes them while the kernel runs.
struct Round {
    int64_t cap0, seg0, lo00, hi00;               // control block: capacity, leaf size, density bounds of the leaf level
    int ema_prev, min_prefix;                     // RoundState::ema / min_prefix
    int64_t rounds_prev, par_ops_prev, deferred_prev;
    // the window of this round (written by the previous round's resolve step, committed by this one's): the pending ops — deferred by
    // earlier rounds, ascending op index — followed by fresh ops
    int64_t i0;                                   // first fresh op
    int np, cur;                                  // pending ops in front of the window, and which half of DevBufs::pend lists them
    int run_ahead, drain;
    int G;                                        // ops of the window
    const PendOp* pend;
    __device__ __forceinline__ int64_t op_index(int q) const { return q < np ? pend[q].op : i0 + (q - np); }
};
__device__ __forceinline__ Round pb_round_load(const DevBufs& db, const Ctl* ctl, const RoundState* rs) {
    Round R;
    R.cap0 = ctl->capacity; R.seg0 = ctl->segment_capacity; R.lo00 = ctl->lo[0]; R.hi00 = ctl->hi[0];
    R.ema_prev = rs->ema; R.min_prefix = rs->min_prefix;
    R.rounds_prev = rs->rounds; R.par_ops_prev = rs->par_ops; R.deferred_prev = rs->deferred;
    R.i0 = rs->cursor_n;
    R.np = rs->np_n; R.cur = rs->cur_n; R.drain = rs->drain;
    const int run_ahead_rs = rs->run_ahead;
    R.pend = db.pend + (size_t)R.cur * PB_GMAX;
    const int64_t left = R.drain ? 0 : (rs->limit - R.i0 > 0 ? rs->limit - R.i0 : 0);
    {
        int Gt = rs->G > R.np ? rs->G : R.np;             // the pending ops are always part of the window
        if (Gt > PB_GMAX) Gt = PB_GMAX;
        const int64_t avail = (int64_t)R.np + left;
        R.G = (int)(avail < Gt ? avail : Gt);
    }
    // (short windows — a small, fast-growing array whose ops collide all the time: config 5's first batches plan ~60 ops a round — are the
    //  prefix rule's: sealing costs the resolve step more than the few ops behind the first conflict are worth; pending ops keep the mode on)
    R.run_ahead = run_ahead_rs && (R.G >= 128 || R.np > 0) ? 1 : 0;
    return R;
}

// ---- the spatial hash -------------------------------------------------------------------------------------------------------------------
// Footprints travel as 32-bit pairs (arrays beyond 2^31 slots: in units of 2^shift slots, rounded outwards — conservative).
// Cell size: 2 * PB_MAX_W slots on large arrays; on a small array ~1/128 of it (not below the leaf, not below 64 slots) — with 4096-slot
// cells every op of a 32 k-slot array is chained into the same few buckets and each walk visits the whole window (config 5's first
// batch: 26 k cycles of the resolve step for 83 planned ops).  Footprints over more than two cells go to the list of wide ops.
constexpr int RS_NB = 4096;                       // buckets
struct Cells {
    int shift, CS;                                // a slot s lies in cell (s >> shift) >> CS
    __device__ __forceinline__ static int bucket(int cell) { return (int)(((uint32_t)cell * 0x9E3779B1u) >> 20) & (RS_NB - 1); }
};
__device__ __forceinline__ Cells pb_cells(int64_t cap0, int64_t seg) {
    constexpr int CS_MAX = PB_MAX_W_LOG2 + 1;
    Cells hc{0, CS_MAX};
    while ((cap0 >> hc.shift) > 0x7fffffffll) ++hc.shift;
    const int lgcap = 63 - __clzll((unsigned long long)(cap0 > 1 ? cap0 : 1)), lgseg = 63 - __clzll((unsigned long long)(seg > 1 ? seg : 1));
    int c = lgcap - 7;
    if (c < lgseg) c = lgseg;
    if (c < 6) c = 6;
    if (hc.shift == 0 && c < CS_MAX) hc.CS = c;
    return hc;
}

// ---- the LDS state ----------------------------------------------------------------------------------------------------------------------
constexpr int RA_MAX_CONF = 96;                   // conflicting ops a round seals at most (more: the prefix rule)
struct alignas(8) Iv { int32_t lo, hi; };
struct Zone { int32_t lo, mid, hi; };             // [A, B] + [B + 1, B + W]: lo = A, mid = B, hi = B + W (lo = 0: no zone)
struct Resolve {
    int sLast;                                    // this workgroup took the last ticket: it resolves the round
    int sC, sB;                                   // smallest op the round is cut at by a conflict / first BARRIER op (G: none)
    int sSumDn, sSumRebN;                         // applied ops: sum of sDn, number of rebalances
    unsigned int sSumRebW;                        // ... and the slots of their windows
    Iv sIv[PB_GMAX + 8];                          // footprints as 32-bit pairs
    int32_t sChg[PB_GMAX];                        // slot whose occupancy the op changes (0: none), exact: tight mode needs shift == 0
    int32_t sChg2[PB_GMAX];                       // the second gap a leaf-accepted new column fills (0: none)
    signed char sDl[PB_GMAX];                     // +1 insert, -1 delete, 0 otherwise
    unsigned char sLvl[PB_GMAX];                  // level of the window a leaf-only op falls back to (0 unless a new column)
    signed char sDn[PB_GMAX];                     // what an insert / delete adds to Ctl::nb_elements (a new column counts for itself in k_apply)
    unsigned short sRebW[PB_GMAX];                // slots of the window an insert / delete rebalances (0: none)
    signed char sCnt02[PB_GMAX];                  // cells of the NEXT leaf if the op needs that one to accept as well (-1: no)
    int32_t sLeafLo[PB_GMAX];                     // first slot of the op's leaf if it is leaf-only, else 0
    int32_t sCnt0[PB_GMAX];                       // cells of that leaf before the round
    // run-ahead: ops that conflict with an earlier op (sConf), ops deferred because they lie in the sealed zone of an earlier deferred op
    // (sDefer), the zone a deferred op is sealed in (sZid -> sZone; 0: none), which ops are plain writes (sSimple: nothing but a hull and
    // their leaf's count ties them to the array), the compact list of the conflicting ops
    unsigned char sAct[PB_GMAX], sConf[PB_GMAX], sDefer[PB_GMAX], sSimple[PB_GMAX];
    unsigned char sZid[PB_GMAX];                  // zone the op is sealed in: 1 + index into the zone table (0: none)
    Zone sZone[RA_MAX_CONF];                      // ... of the q-th conflicting op (owner sConfList[q])
    int sConfList[RA_MAX_CONF];
    int sNConf, sNApplied, sNDeferred, sFault;
    uint32_t sScan[PL_BLOCK / 64];                // next window: kept ops per wave
    int sHead[RS_NB];                             // spatial hash: first entry of a bucket's chain (-1: empty); entry e = 2 * op + (0: its first cell, 1: its second)
    int sNext[2 * PB_GMAX];                       // ... and the entry behind entry e
    int sWide[PB_GMAX];                           // ops tested against everybody: footprints over more than two cells, widened ops that left their cells
    int sNWide;
    int64_t sLoH[24], sHiH[24];                   // density bounds of the lower levels (run-ahead: the sealed zones)
    int sMinConf;                                 // smallest conflicting op (run-ahead; INT32_MAX: none)
    int sSealList[PL_BLOCK / 64][64];             // seal: per wave, the ops that touch the region its candidate zones lie in
#ifdef DSA_PB_PROF
    unsigned char sCutWhy[PB_GMAX + 8];           // dev profile: what cut the round at op j (see dsa_dbg_pbprof_dump)
#endif
};

// ---- stage 1, load -----------------------------------------------------------------------------------------------------------------------
// Reads:  the plans of the window (device-scope loads: they were published by other workgroups), Ctl::lo / hi under run-ahead.
// Writes: the per-op records (sAct .. sCnt0) and the 32-bit footprints sIv of ops [0, G) (+ 8 empty ones), sB = first BARRIER; empties
//         the hash (sHead) and the run-ahead state under the latency of the plan loads.
// A barrier follows: the chain stage reads sB and every footprint.
__device__ __forceinline__ void resolve_load(Resolve& S, const Round& R, const Cells hc, const Ctl* ctl, const Plan* plans) {
    const int tid = threadIdx.x, G = R.G, shift = hc.shift;
    const int64_t seg = R.seg0;
    if (R.run_ahead && tid >= PL_BLOCK - 24) { const int q = tid - (PL_BLOCK - 24); S.sLoH[q] = ctl->lo[q]; S.sHiH[q] = ctl->hi[q]; }      // (the LAST wave: fewest plans to load)
    // (spatial hash of the overlap test; emptied here, under the latency of the plan loads, behind the same barrier)
    for (int k = tid; k < RS_NB; k += PL_BLOCK) S.sHead[k] = -1;
    if (tid == 0) { S.sNWide = 0; S.sNConf = 0; S.sNApplied = 0; S.sNDeferred = 0; S.sFault = 0; S.sMinConf = INT32_MAX; }
    for (int j = tid; j < G + 8 && j < PB_GMAX; j += PL_BLOCK) { S.sConf[j] = 0; S.sDefer[j] = 0; S.sSimple[j] = 0; S.sZid[j] = 0; S.sAct[j] = PB_BARRIER; }
    if (tid < RA_MAX_CONF) { S.sZone[tid].lo = 0; S.sZone[tid].mid = 0; S.sZone[tid].hi = 0; }
    for (int j = tid; j < G + 8; j += PL_BLOCK) {
        Iv iv{INT32_MAX, INT32_MIN};                                   // an empty footprint overlaps nothing
        if (j < G) {
            const Plan* q = plans + j;
            const int64_t lo = __hip_atomic_load(&q->lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int64_t hi = __hip_atomic_load(&q->hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int64_t ws = __hip_atomic_load(&q->ws, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int64_t we = __hip_atomic_load(&q->we, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int64_t pos = __hip_atomic_load(&q->pos, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int64_t aux = __hip_atomic_load(&q->aux, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int32_t cnt = __hip_atomic_load(&q->count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int32_t act = __hip_atomic_load(&q->action, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (act == PB_BARRIER) atomicMin(&S.sB, j);
            S.sAct[j] = (unsigned char)act;
            const bool leaf_only = pb_is_leaf_only(act, ws, we, seg, cnt);
            const int dl = pb_delta(act, leaf_only);
            const int64_t chg = pb_changed_slot(act, pos, aux);
            const bool newcol = act == PB_NEWCOL;
            S.sDl[j] = (signed char)dl;
            S.sChg[j] = (dl != 0 && shift == 0) ? (int32_t)chg : 0;
            S.sChg2[j] = (newcol && leaf_only && shift == 0) ? (int32_t)hi : 0;
            S.sLvl[j] = newcol ? (unsigned char)(cnt & 0x7f) : 0;
            const bool insdel = act == PB_INS_R || act == PB_INS_L || act == PB_DELETE;
            S.sDn[j] = insdel ? (signed char)(act == PB_DELETE ? -1 : 1) : (signed char)0;
            S.sRebW[j] = (insdel && we - ws + 1 != seg) ? (unsigned short)(we - ws + 1) : (unsigned short)0;      // (<= PB_MAX_W)
            int64_t flo = lo, fhi = hi;
            if (leaf_only && shift == 0) {
                S.sLeafLo[j] = newcol ? (int32_t)((pos / seg) * seg + 1) : (int32_t)ws;      // (new column: the leaf of pos + 1, its semaphore)
                S.sCnt0[j] = newcol ? ((cnt >> 8) & 0x7f) : cnt - ((chg >= ws && chg <= we) ? dl : 0);
                S.sCnt02[j] = (newcol && (cnt & 0x8000)) ? (signed char)((cnt >> 16) & 0x7f) : (signed char)-1;
            } else {
                S.sLeafLo[j] = 0; S.sCnt0[j] = 0;
                if (leaf_only && lo <= hi) { if (ws < flo) flo = ws; if (we > fhi) fhi = we; }      // (arrays beyond 2^31 slots: always the window)
            }
            if (flo <= fhi) { iv.lo = (int32_t)(flo >> shift); iv.hi = (int32_t)(fhi >> shift); }
        }
        S.sIv[j] = iv;
    }
}

// ---- stage 2, chain ----------------------------------------------------------------------------------------------------------------------
// Smallest j that overlaps an earlier op: a spatial hash instead of all pairs (G^2 / 2 tests by one workgroup cost 7 .. 36 us).
// A footprint of up to a cell's size lies in one or two cells and is chained into their buckets, then every op walks the chains of its
// own cells and tests the earlier ops it meets there exactly.  The (rare) longer footprints are tested against everybody.  Ops at or
// behind the first BARRIER do not matter: Gc = min(sB, G) ops are chained.
// Reads:  sIv.   Writes: sHead / sNext (the chains), sWide / sNWide.
// A barrier follows: the walks of the next stage read the finished chains.
__device__ __forceinline__ void resolve_chain(Resolve& S, const Cells hc, const int Gc) {
    const int CS = hc.CS;
    for (int j = threadIdx.x; j < Gc; j += PL_BLOCK) {
        const Iv iv = S.sIv[j];
        if (iv.lo > iv.hi) continue;
        const int c0 = iv.lo >> CS, c1 = iv.hi >> CS;
        if (c1 - c0 > 1) { S.sWide[atomicAdd(&S.sNWide, 1)] = j; continue; }
        for (int k = 0; k <= c1 - c0; ++k) { const int e = 2 * j + k; S.sNext[e] = atomicExch(&S.sHead[hc.bucket(c0 + k)], e); }
    }
}

// what op i adds to the inserts into / deletes from the slots [a, b]
__device__ __forceinline__ void resolve_tally(const Resolve& S, int i, int32_t a, int32_t b, int& ins, int& del) {
    const int32_t ch = S.sChg[i], ch2 = S.sChg2[i];
    if (ch >= a && ch <= b) { if (S.sDl[i] > 0) ++ins; else ++del; }
    if (ch2 >= a && ch2 <= b) ++ins;
}
// does the leaf [a, a + seg) with c cells before the round accept every count the window's ops can leave in it?  (nwide: the wide ops
// of the chain stage)
__device__ __forceinline__ bool resolve_leaf_accepts(const Resolve& S, const Round& R, const Cells hc, int nwide, int32_t a, int64_t c) {
    const int CS = hc.CS;
    const int32_t b = a + (int32_t)R.seg0 - 1;
    int ins = 0, del = 0;
    // The cells the leaf lies in.  Slots are 1-based, leaves start at k * seg + 1: the LAST slot of a leaf is a multiple of seg
    // and, once in 2^CS / seg leaves, the first slot of the next cell — an op that changes that slot is chained THERE, not in
    // the cell of the leaf's first slot (round 2-4 walked only that one: two deletes from one leaf, one of them of its last
    // slot 237568 = 116 * 2048, ran in one round and left the leaf empty without the rebalance; tools/fuzz.py, FUZZ_BIG seed 91098).
    const int cl0 = a >> CS, cl1 = DSA_FP_REGRESS == 1 ? cl0 : b >> CS;
    for (int cl = cl0; cl <= cl1; ++cl) {
        if (cl != cl0 && hc.bucket(cl) == hc.bucket(cl0)) break;      // the same chain again
        for (int e = S.sHead[hc.bucket(cl)]; e >= 0; e = S.sNext[e]) {
            const int i = e >> 1;
            const int first = S.sIv[i].lo >> CS;
            if ((e & 1) && first == cl) continue;               // an op chained twice into this bucket's cell is counted once
            if (cl != cl0 && first == cl0) continue;            // ... and so is an op whose hull lies in both cells of the leaf
            resolve_tally(S, i, a, b, ins, del);
        }
    }
    for (int w2 = 0; w2 < nwide; ++w2) resolve_tally(S, S.sWide[w2], a, b, ins, del);
    return c + ins <= R.hi00 && c - del >= R.lo00;
}

// ---- stage 3, leaf counts ----------------------------------------------------------------------------------------------------------------
// Ops accepted by their LEAF move nothing but their shifted run; what else ties two of them together is the leaf's cell COUNT
// (src/pma.jl:118-126).  If the leaf accepts the count whatever subset of the window's ops has changed it — count0 + all inserts
// into the leaf <= hi[0], count0 - all deletes >= lo[0] — every order of those ops takes the same decisions, and the op's
// footprint is just its tight hull (predecessor .. filled gap): two inserts into one 16-slot leaf no longer collide, only
// overlapping runs do.  Otherwise the footprint is widened to the leaf, as for every op with a wider window.  (Round 2 always
// used the leaf: conflict-free prefixes of ~250 ops on a 2^21-slot array, birthday-bound by 16-slot footprints.)
// The sums per leaf come from a walk of the same spatial hash the overlap test uses: an op that changes the count of leaf L
// has the changed slot in its hull, so it is chained in the cell of L.
// Leaf-only ops: inserts into / deletes from their leaf by ANY op of the window in front of the first BARRIER (themselves included);
// the leaf must accept every count in between, else the footprint is widened to the leaf.
// Reads:  the chains, sIv (the TIGHT hulls), the per-op records, RoundState::tight.
// Writes: sIv of the widened ops (behind the barrier inside: every walk has read the tight hulls by then), sWide / sNWide (widened ops
//         that left their cells), sSimple, sC (a new column that cannot be widened).
// A barrier follows: the overlap walks read the final footprints.
__device__ __forceinline__ void resolve_leaf_counts(Resolve& S, const Round& R, const Cells hc, const int Gc, const RoundState* rs) {
    const int tid = threadIdx.x, CS = hc.CS;
    const int64_t seg = R.seg0;
    const int nwide0 = S.sNWide;
    const int tight_mask = rs->tight;
    bool widen[PB_GMAX / PL_BLOCK];
#pragma unroll
    for (int u = 0; u < PB_GMAX / PL_BLOCK; ++u) {
        const int j = tid + u * PL_BLOCK;
        widen[u] = false;
        if (j >= Gc) continue;
        const int32_t l0 = S.sLeafLo[j];
        if (l0 == 0) continue;
        const Iv me = S.sIv[j];
        const int c0 = me.lo >> CS, c1 = me.hi >> CS;
        if (c1 - c0 > 1) {                                           // (a tight hull over three cells: keep it simple)
            // ... a new column without a fallback window (level 0x7f) has nothing to be widened to: W = seg << 0x7f below is undefined.
            // The prefix ends in front of it, like further down
            if (S.sLvl[j] == 0x7f) { PBW(S, j, 9); atomicMin(&S.sC, j); } else widen[u] = true;
            continue;
        }
        bool ok = resolve_leaf_accepts(S, R, hc, nwide0, l0, S.sCnt0[j]);
        if (ok && S.sCnt02[j] >= 0) ok = resolve_leaf_accepts(S, R, hc, nwide0, l0 + (int32_t)seg, S.sCnt02[j]);
        widen[u] = !ok || !((tight_mask >> (S.sChg2[j] != 0 ? 1 : 0)) & 1);
        // a new column without a fallback window (level 0x7f) cannot be widened: the prefix ends in front of it (alone at the head
        // of the next round it is handed to the sequencer — d = 0 stops the rounds)
        if (widen[u] && S.sLvl[j] == 0x7f) { widen[u] = false; PBW(S, j, 9); atomicMin(&S.sC, j); }
        // "simple" (run-ahead): a leaf-accepted right insert / delete that keeps its tight hull
        if (!widen[u] && (S.sAct[j] == PB_INS_R || S.sAct[j] == PB_DELETE)) S.sSimple[j] = 1;
    }
    __syncthreads();                                               // every walk has read the tight hulls
#pragma unroll
    for (int u = 0; u < PB_GMAX / PL_BLOCK; ++u) {
        const int j = tid + u * PL_BLOCK;
        if (j < Gc && widen[u]) {
            Iv me = S.sIv[j];
            // back to the window the plan was accepted in: the leaf, or the level-H window of a new column
            const int32_t W = (int32_t)seg << S.sLvl[j];
            const int32_t a = ((S.sLeafLo[j] - 1) / W) * W + 1, b = a + W - 1;
            const int oc0 = me.lo >> CS, oc1 = me.hi >> CS;                  // the cells the op is chained in (its tight hull)
            if (a < me.lo) me.lo = a;
            if (b > me.hi) me.hi = b;
            // The widened interval can reach into a cell the op is not chained in — slots are 1-based, an aligned window ends on a multiple
            // of its size, e.g. [516081, 516096] with 516096 = 126 * 4096 the first slot of the next cell.  For a leaf-accepted insert /
            // delete that is harmless (it writes only its tight hull; the widening stands for the count it read), but a widened NEW COLUMN
            // scans and REBALANCES its whole window when it is applied: a later op that starts on that last slot walked only its own cell
            // and ran in the same round (rounds 3-4; found by the footprint-check build of round 5, tools/fuzz.py run_same_leaf_matrix,
            // first seed 9101: "op 52 writes inside [516081,516096]; the later op 54 has the footprint [516096,516098]").  Such an op is
            // tested against everybody, like the footprints longer than two cells.
            if (DSA_FP_REGRESS != 3 && ((me.lo >> CS) != oc0 || (me.hi >> CS) != oc1)) S.sWide[atomicAdd(&S.sNWide, 1)] = j;
            S.sIv[j] = me;
        }
    }
}

// ---- stage 4, overlaps -------------------------------------------------------------------------------------------------------------------
// Every op against the EARLIER ops in the chains of its own cells, then (behind the barrier inside) the wide ops against everybody.
// Reads:  the chains, sWide, the final sIv.
// Writes: the prefix rule: sC = smallest op that overlaps an earlier one; run-ahead: sConf marks and sMinConf instead.
// A barrier follows: the seal and decide stages read sC / sConf / sMinConf.
__device__ __forceinline__ void resolve_overlaps(Resolve& S, const Round& R, const Cells hc, const int Gc) {
    const int tid = threadIdx.x, CS = hc.CS, run_ahead = R.run_ahead;
    for (int j = tid; j < Gc; j += PL_BLOCK) {
        const Iv me = S.sIv[j];
        if (me.lo > me.hi) continue;
        const int c0 = me.lo >> CS, c1 = me.hi >> CS;
        if (c1 - c0 > 1) continue;
        bool hit = false;
        for (int k = 0; k <= c1 - c0; ++k)
            for (int e = S.sHead[hc.bucket(c0 + k)]; e >= 0; e = S.sNext[e]) {
                const int i = e >> 1;
                const Iv o = S.sIv[i];
                hit = hit | ((i < j) & (o.lo <= me.hi) & (me.lo <= o.hi));
            }
        if (hit) { if (run_ahead) { S.sConf[j] = 1; atomicMin(&S.sMinConf, j); } else { PBW(S, j, 1); atomicMin(&S.sC, j); } }
    }
    __syncthreads();
    const int nwide = S.sNWide;
    for (int w = 0; w < nwide; ++w) {
        const int j = S.sWide[w];
        const Iv me = S.sIv[j];
        for (int i = tid; i < Gc; i += PL_BLOCK) {
            const Iv o = S.sIv[i];
            if (i != j && o.lo <= me.hi && me.lo <= o.hi) { if (run_ahead) { S.sConf[i > j ? i : j] = 1; atomicMin(&S.sMinConf, i > j ? i : j); } else { PBW(S, i > j ? i : j, 1); atomicMin(&S.sC, i > j ? i : j); } }
        }
    }
}

// visits every op of the window whose footprint overlaps [a, b] (an op in two cells of the walk once; a widened op that is also in
// the list of wide ops twice — the counts of the seal stage are upper bounds)
template <class F>
__device__ __forceinline__ void resolve_for_overlapping(const Resolve& S, const Cells hc, int64_t a, int64_t b, F fn) {
    const int CS = hc.CS;
    const int ca = (int)(a >> CS), cb = (int)(b >> CS);
    for (int cl = ca; cl <= cb; ++cl)
        for (int e = S.sHead[hc.bucket(cl)]; e >= 0; e = S.sNext[e]) {
            const int i = e >> 1;
            const Iv o = S.sIv[i];
            const int ci = (o.lo >> CS) + (e & 1);                 // the cell this entry stands for
            if (ci != cl) continue;                               // (another cell of the same bucket)
            if ((e & 1) && (o.lo >> CS) >= ca) continue;          // the op's first cell lies in the walked range too: visited there
            if (o.lo <= b && a <= o.hi) fn(i);
        }
    const int nw = S.sNWide;
    for (int q = 0; q < nw; ++q) { const int i = S.sWide[q]; const Iv o = S.sIv[i]; if (o.lo <= b && a <= o.hi) fn(i); }
}

// ---- stage 5, seal (run-ahead only) ------------------------------------------------------------------------------------------------------
// Reads:  sConf / sMinConf, the chains, sIv, sAct, sLoH / sHiH, the occupancy bitmap around the conflicting ops.
// Writes: sSimple ("plain write" from here on), sConfList / sNConf, sZone, sZid, sDefer, and sC wherever a zone cannot be proven.
// Every path that writes ends with a barrier of its own: the decide stage follows without one in between.
__device__ __forceinline__ void resolve_seal(Resolve& S, const Round& R, const Cells hc, const int Gc, const Ctl* ctl, const uint64_t* occ,
                                             const RoundState* rs) {
    if (!R.run_ahead || S.sMinConf == INT32_MAX) return;
    const int tid = threadIdx.x, shift = hc.shift;
    const int64_t seg = R.seg0, cap0 = R.cap0;
    // Sealing costs the resolving workgroup a few dependent round trips to memory per round; it does not pay when the first conflict
    // sits in the last eighth of the window anyway (a long prefix: the array is large against the window): the prefix rule then
    if (S.sMinConf >= Gc - (Gc >> 3)) {
        if (tid == 0) { PBW(S, S.sMinConf, 2); atomicMin(&S.sC, S.sMinConf); }
        __syncthreads();
        return;
    }
    // ---- run-ahead: which conflicting ops can be DEFERRED without holding back the ops behind them --------------------------------
    // An op j that conflicts with an earlier one is deferred to the next round.  Ops behind it may still run in THIS round if nothing
    // that j can touch when it is finally executed — on the state its earlier partners leave, which is not the state it was planned
    // on — is theirs.  j is SEALED in a zone Z' = [A, B] + [B + 1, B + W]: the aligned window of some level h (W = seg << h slots,
    // 64 <= W <= RA_MAX_W) that holds j's footprint and the footprints of the earlier ops it overlaps, plus the window to its right,
    // such that
    //   (0) more than D cells lie between A and the leftmost op inside (a predecessor moves left by one cell per deleted cell: it
    //       stays inside);
    //   (1) every op of the round's window that touches Z' lies inside [A, B] and is a plain write (overwrite, missing-key delete,
    //       right-shifting insert, delete; whatever window <= [A, B] its density scan was planned to rebalance) or a new column IN
    //       FRONT of j (applied in this round: a semaphore + its first element, two inserts): I potential inserts (every op with a
    //       value, two per new column), D potential deletes (every op without);
    //   (2) both windows accept at level h whatever those ops do: lo[h] <= c - D and c + I <= hi[h] for the cell counts c of
    //       [A, B] and of [B + 1, B + W]: no density scan at a position inside Z' climbs above level h, rebalances stay inside;
    //   (3) the right window keeps more than I + 1 gaps (W - hi[h] >= I + 2): an insert position can drift right by one slot per
    //       earlier insert, to B + 1 + I at most, and a gap is left beyond it: every shifted run ends inside Z', nobody takes the
    //       left branch of _insert!.
    // So whatever happens in Z' from now on stays in Z', and Z' is touched by nobody else: ops behind j that lie inside [A, B] are
    // deferred with it (in order), ops that touch Z' otherwise end the round in front of them (prefix rule from there), and
    // everything else is applied.  The zone travels with the pending op (PendOp); when the op is applied its footprint must lie
    // inside it — checked by the decide stage, a violation fails the batch instead of diverging from the sequential order.  Whatever
    // cannot be proven (no level fits, a new column or a left-shifting insert nearby, arrays beyond 2^31 slots) cuts the round at j.
    constexpr int RA_MAX_W = 1024, RA_MAX_DEL = 8;
    for (int j = tid; j < Gc; j += PL_BLOCK) {
        const int a = S.sAct[j];
        S.sSimple[j] = (a == PB_OVERWRITE || a == PB_NOOP || a == PB_INS_R || a == PB_DELETE) ? 1 : 0;      // "plain write"
        if (S.sConf[j]) { const int q = atomicAdd(&S.sNConf, 1); if (q < RA_MAX_CONF) S.sConfList[q] = j; }
    }
    __syncthreads();
    // (a window full of conflicts — hammering one leaf, a tiny array — is the prefix rule's: most zones would not hold anyway)
    const int nconf = S.sNConf > RA_MAX_CONF ? 0 : S.sNConf;
    if (S.sNConf > RA_MAX_CONF && tid == 0) { PBW(S, S.sMinConf, 3); atomicMin(&S.sC, S.sMinConf); }
    // one WAVE per conflicting op, ONE pass for all candidate levels: every zone a level could offer lies inside R = the aligned window
    // of the widest level (RA_MAX_W slots) plus the window to its right.  Lane 0 walks the hash chains of R once and lists the ops it
    // meets (one per lane from then on), lanes 0..31 load R's occupancy words in one round and a prefix sum over their popcounts
    // gives the cell count of any aligned window; the levels are then tried narrowest first without touching memory again.  (Round 6's
    // first form walked the chains and loaded the words once per level: 13-47 k cycles of the resolve step for 1-7 conflicts.)
    {
        const int lane = tid & 63, wave = tid >> 6;
        for (int q = wave; q < nconf; q += PL_BLOCK / 64) {
            const int j = S.sConfList[q];
            const Iv me = S.sIv[j];
            bool ok = shift == 0 && S.sSimple[j] && me.lo <= me.hi && me.lo >= 1;
            int64_t A = 0, B = 0, W = 0;
            int64_t a = me.lo, b = me.hi;
            if (ok && lane == 0)
                resolve_for_overlapping(S, hc, me.lo, me.hi, [&](int i) { if (i < j) { const Iv o = S.sIv[i]; if (o.lo < a) a = o.lo; if (o.hi > b) b = o.hi; } });
            a = __shfl(a, 0, 64); b = __shfl(b, 0, 64);
            int hmin = -1, hmax = -1, n = 0;
            for (int h = 0; h < MAX_LEVELS; ++h) {
                const int64_t Wh = seg << h;
                if (Wh < 64) continue;
                if (Wh > RA_MAX_W) break;
                if (hmin < 0) hmin = h;
                hmax = h;
            }
            if (ok && hmax >= 0) {
                ok = false;
                const int64_t Wx = seg << hmax;
                const int64_t Ax = ((a - 1) / Wx) * Wx + 1;
                const int64_t Rhi = Ax + 2 * Wx - 1 < cap0 ? Ax + 2 * Wx - 1 : cap0;          // R = [Ax, Rhi]: whole words (64 | Wx, 64 | cap0)
                if (lane == 0) resolve_for_overlapping(S, hc, Ax, Rhi, [&](int i) { if (n < 64) S.sSealList[wave][n] = i; ++n; });
                n = __shfl(n, 0, 64);
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                // the ops that touch R, one per lane (more than 64: nothing is proven, the round ends in front of j)
                Iv o{INT32_MAX, INT32_MIN};
                bool osimple = false, oins = false, onew = false;
                if (n <= 64 && lane < n) {
                    const int i = S.sSealList[wave][lane];
                    o = S.sIv[i]; osimple = S.sSimple[i] != 0; oins = S.sAct[i] == PB_OVERWRITE || S.sAct[i] == PB_INS_R;
                    // an EARLIER new column (applied in this round — if it conflicted itself the round would end in front of it): a
                    // semaphore and its first element, two right-shifting inserts as far as the zone is concerned
                    onew = S.sAct[i] == PB_NEWCOL && i < j;
                }
                // the occupancy words of R and the inclusive prefix sum of their popcounts (lane t <-> word t of R)
                const int64_t w0 = (Ax - 1) >> 6;
                const int nwR = (int)((Rhi - Ax + 1) >> 6);                                   // <= 32
                const uint64_t word = (n <= 64 && lane < nwR) ? occ[w0 + lane] : 0ull;
                int incl = popc64(word);
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) { const int up = __shfl_up(incl, d, 64); if (lane >= d) incl += up; }
                auto cells_before = [&](int k) -> int { const int v = __shfl(incl, k > 0 ? k - 1 : 0, 64); return k > 0 ? v : 0; };      // words [0, k) of R
                for (int h = hmin; n <= 64 && h <= hmax; ++h) {
                    W = seg << h;
                    A = ((a - 1) / W) * W + 1; B = A + W - 1;
                    if (b > B) continue;
                    if (B + W > cap0) break;
                    // (1) every op that touches Z' lies inside [A, B] and is a plain write
                    const bool ov = o.lo <= B + W && A <= o.hi;                               // (an idle lane's empty interval overlaps nothing)
                    const uint64_t ovm = __ballot(ov);
                    if (__ballot(ov && (!(osimple || onew) || o.lo < A || o.hi > B)) != 0ull) continue;
                    const int nins = popc64(__ballot(ov && oins)), nnew = popc64(__ballot(ov && onew));
                    const int ins = nins + 2 * nnew, del = popc64(ovm) - nins - nnew;
                    if (del > RA_MAX_DEL) continue;
                    const int64_t lh = h < 24 ? S.sLoH[h] : ctl->lo[h], hh = h < 24 ? S.sHiH[h] : ctl->hi[h];
                    if (W - hh < ins + 2) continue;
                    int min_lo = ov ? o.lo : INT32_MAX;
#pragma unroll
                    for (int d = 32; d > 0; d >>= 1) { const int other = __shfl_xor(min_lo, d, 64); min_lo = other < min_lo ? other : min_lo; }
                    const int wl = (int)(((A - 1) >> 6) - w0), nwd = (int)(W >> 6);
                    const int c_a = cells_before(wl), c_b = cells_before(wl + nwd), c_c = cells_before(wl + 2 * nwd);
                    const int64_t cl = c_b - c_a, cr = c_c - c_b;
                    // (0) a predecessor moves left by one cell per deleted cell: more than `del` cells lie between A and the leftmost op
                    int64_t cm = 0;
                    const int64_t m1 = (int64_t)min_lo - 2;                                   // 0-based slots [A - 1, min_lo - 2]
                    if (min_lo != INT32_MAX && m1 >= A - 1) {
                        const int kw = (int)((m1 >> 6) - w0);
                        const uint32_t wlo = (uint32_t)__shfl((int)(uint32_t)word, kw, 64), whi = (uint32_t)__shfl((int)(uint32_t)(word >> 32), kw, 64);
                        const uint64_t wk = ((uint64_t)whi << 32) | wlo;
                        const int r = (int)(m1 & 63);
                        cm = cells_before(kw) - c_a + popc64(r == 63 ? wk : (wk & ((1ull << (r + 1)) - 1ull)));
                    }
                    if (cm < del + 1) continue;
                    if (lh <= cl - del && cl + ins <= hh && lh <= cr - del && cr + ins <= hh) { ok = true; break; }
                }
            } else ok = false;
            if (lane == 0) {
                if (ok) {
                    fp_note_sealed(rs, (long long)R.op_index(j), j, (int)S.sAct[j], me.lo, me.hi, (long long)A, (long long)B, (long long)W);
                    S.sZone[q].lo = (int32_t)A; S.sZone[q].mid = (int32_t)B; S.sZone[q].hi = (int32_t)(B + W);
                }
                else { PBW(S, j, !S.sSimple[j] ? 5 : (n > 64 ? 4 : 6)); atomicMin(&S.sC, j); }                                                    // not provable: the round ends in front of this op
            }
        }
    }
    __syncthreads();
    // zones must not touch each other: a later conflicting op inside the left window of an earlier zone is a member of that one,
    // otherwise the round ends at it
    for (int q = tid; q < nconf; q += PL_BLOCK) {
        const Zone zq = S.sZone[q];
        if (zq.lo == 0) continue;
        const int j = S.sConfList[q];
        const Iv me = S.sIv[j];
        bool member = false, cut = false;
        for (int r = 0; r < nconf; ++r) {
            const int i = S.sConfList[r];
            const Zone zr = S.sZone[r];
            if (i >= j || zr.lo == 0) continue;
            if (zr.lo <= zq.hi && zq.lo <= zr.hi) { if (me.lo >= zr.lo && me.hi <= zr.mid) member = true; else cut = true; }
        }
        if (cut) { PBW(S, j, 7); atomicMin(&S.sC, j); }
        else if (member) S.sDefer[j] = 2;                                            // (its own zone is dropped below, behind the barrier)
    }
    __syncthreads();
    for (int q = tid; q < nconf; q += PL_BLOCK) { if (S.sDefer[S.sConfList[q]] == 2) S.sZone[q].lo = 0; else if (S.sZone[q].lo != 0) S.sZid[S.sConfList[q]] = (unsigned char)(q + 1); }
    __syncthreads();
    // every op behind a sealed op: inside the left window of the zone -> deferred with it; touching the zone otherwise -> the round ends there
    for (int x = tid; x < Gc; x += PL_BLOCK) {
        const Iv me = S.sIv[x];
        if (me.lo > me.hi) continue;
        int zid = 0;
        for (int r = 0; r < nconf; ++r) {
            const Zone zr = S.sZone[r];
            if (S.sConfList[r] >= x || zr.lo == 0) continue;
            if (me.lo <= zr.hi && zr.lo <= me.hi) {
                if (me.lo >= zr.lo && me.hi <= zr.mid && S.sSimple[x]) { if (zid == 0) zid = r + 1; }
                else { PBW(S, x, 8); atomicMin(&S.sC, x); }
            }
        }
        if (zid != 0) { if (!S.sDefer[x]) S.sDefer[x] = 1; if (S.sZid[x] == 0) S.sZid[x] = (unsigned char)zid; }      // (only x's own entries: the owners' zones are final)
    }
    __syncthreads();
}

// ---- stage 6, decide ---------------------------------------------------------------------------------------------------------------------
// The decision: ops [0, dd) are looked at; of those, the ones that neither conflict with an earlier op nor are sealed behind one are
// applied by k_apply; the others go (in order) to the pending list of the next round, in front of the fresh ops.
// Reads:  sC, sB, sConf, sDefer, sDn, sRebW, sIv, sAct, the zones the pending ops carry.
// Writes: sSumDn / sSumRebN / sSumRebW, sNApplied, sNDeferred, sFault; behind the barrier inside, the verdict every thread holds.
struct Verdict {
    int dd;                                       // ops [0, dd) of the window are decided by this round
    int na, ema;                                  // applied ops, and the running average of that (x16)
    bool stop_short;                              // the rounds stop here: the sequencer takes the op at the head of the window
};
__device__ __forceinline__ Verdict resolve_decide(Resolve& S, const Round& R) {
    const int tid = threadIdx.x, G = R.G, np = R.np;
    const PendOp* pend = R.pend;
    Verdict V;
    int dd = S.sC < S.sB ? S.sC : S.sB;
    if (dd > G) dd = G;
    V.dd = dd;
    V.stop_short = false;
    {
        // applied ops: element count and rebalance statistics, added to the control block ONCE, by the commit stage (k_apply's waves used
        // to add them one by one: ~500 atomics per round on the same words); zone check of the pending ones
        int dn = 0, rn = 0, na = 0, nd = 0, bad = 0;
        unsigned int rw = 0u;
        const bool plain_round = S.sMinConf == INT32_MAX && np == 0;          // no conflict, nothing pending: every op of [0, dd) is applied
        for (int j = tid; j < dd; j += PL_BLOCK) {
            if (!plain_round && (S.sConf[j] || S.sDefer[j])) { ++nd; continue; }
            ++na;
            dn += S.sDn[j]; const unsigned int w2 = S.sRebW[j]; if (w2) { ++rn; rw += w2; }
            if (j < np) {                                              // deferred earlier: it must still act inside the zone it was sealed in
                const PendOp po = pend[j];
                const Iv me = S.sIv[j];
                if (po.zlo != 0 && S.sAct[j] != PB_NOOP && me.lo <= me.hi && (me.lo < po.zlo || me.hi > po.zhi)) {      // (a missing-key delete writes nothing)
                    bad = 1;
                    fp_note_zone_fault(po, j, np, me.lo, me.hi, (int)S.sAct[j]);
                }
            }
        }
        if (tid == 0 && S.sB == 0 && np > 0 && pend[0].zlo != 0) bad = 1;          // a sealed op that cannot be planned any more
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { dn += __shfl_xor(dn, o, 64); rn += __shfl_xor(rn, o, 64); rw += __shfl_xor(rw, o, 64); }
        if (!plain_round) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { na += __shfl_xor(na, o, 64); nd += __shfl_xor(nd, o, 64); bad |= __shfl_xor(bad, o, 64); }
        }
        if ((tid & 63) == 0) {
            if (dn != 0 || rn != 0) { atomicAdd(&S.sSumDn, dn); atomicAdd(&S.sSumRebN, rn); atomicAdd(&S.sSumRebW, rw); }
            if (plain_round) { if (tid == 0) S.sNApplied = dd; }
            else {
                if (na) atomicAdd(&S.sNApplied, na);
                if (nd) atomicAdd(&S.sNDeferred, nd);
                if (bad) atomicExch(&S.sFault, 1);
            }
        }
    }
    __syncthreads();
    const int na = S.sNApplied;
    const int ema = (3 * R.ema_prev + 16 * na) >> 2;
    V.na = na; V.ema = ema;
    // short rounds one after the other mean the ops around the cursor collide (appends, one hot key): hand over to the
    // sequencer.  A single short round between long ones (a small array, where windows are wide) is still cheaper as a round
    // of >= 1 ops than as a sequencer launch.
    // (with pending ops in the window only an op that cannot be planned stops the rounds: the sequencer takes ONE pending op at a time)
    if (G > 0 && na < R.min_prefix && dd < G && (na == 0 || (np == 0 && ema < 16 * R.min_prefix))) V.stop_short = true;
    if (G <= 0) V.stop_short = false;
    return V;
}

// ---- stage 7, next window ----------------------------------------------------------------------------------------------------------------
// The next window: pending list = the deferred ops of [0, dd) and the pending ops at or behind dd, in window order, each with the zone
// it may still touch (the zone it was sealed in now, intersected with the one it carries).
// Reads:  the verdict, sConf, sDefer, sZid / sZone, sNDeferred, this round's pending list.
// Writes: the other half of DevBufs::pend; sScan (a barrier inside separates the per-wave counts from the offsets).
// No barrier follows: the commit stage publishes only what thread 0 holds itself.
struct NextWindow { int np_next; int64_t cursor_next; };
__device__ __forceinline__ NextWindow resolve_next_window(Resolve& S, const Round& R, const Verdict V, PendOp* pend_next) {
    const int tid = threadIdx.x, G = R.G, np = R.np, dd = V.dd;
    const PendOp* pend = R.pend;
    NextWindow N{np, R.i0};
    const bool any_pending = S.sNDeferred > 0 || np > dd;               // (uniform: LDS word / kernel scalars)
    if (!V.stop_short && G > 0 && !any_pending) { N.np_next = 0; N.cursor_next = R.i0 + (dd > np ? dd - np : 0); }
    if (!V.stop_short && G > 0 && any_pending) {
        // (PB_GMAX / PL_BLOCK consecutive window positions per thread)
        constexpr int NR = PB_GMAX / PL_BLOCK;
        bool keep[NR];
        uint32_t mine = 0;
#pragma unroll
        for (int u = 0; u < NR; ++u) {
            const int j = tid * NR + u;
            keep[u] = j < G && ((j < dd && (S.sConf[j] || S.sDefer[j])) || (j >= dd && j < np));
            mine += keep[u] ? 1u : 0u;
        }
        uint32_t inc = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const uint32_t y = __shfl_up(inc, o, 64); if ((tid & 63) >= o) inc += y; }
        if ((tid & 63) == 63) S.sScan[tid >> 6] = inc;
        __syncthreads();
        uint32_t base = 0, total = 0;
#pragma unroll
        for (int v = 0; v < PL_BLOCK / 64; ++v) { const uint32_t c = S.sScan[v]; if (v < (tid >> 6)) base += c; total += c; }
        uint32_t at = base + inc - mine;
#pragma unroll
        for (int u = 0; u < NR; ++u) {
            if (!keep[u]) continue;
            const int j = tid * NR + u;
            PendOp po;
            po.op = R.op_index(j);
            int32_t zl = 0, zh = 0;
            if (j < dd && S.sZid[j] != 0) { const Zone z = S.sZone[S.sZid[j] - 1]; zl = z.lo; zh = z.hi; }
            if (j < np) {                                              // intersect with the zone it carries
                const PendOp old = pend[j];
                if (old.zlo != 0) { if (zl == 0) { zl = old.zlo; zh = old.zhi; } else { zl = zl > old.zlo ? zl : old.zlo; zh = zh < old.zhi ? zh : old.zhi; } }
            }
            po.zlo = zl; po.zhi = zh;
            pend_next[at++] = po;
        }
        N.np_next = (int)total;
        N.cursor_next = R.i0 + (dd > np ? dd - np : 0);
    }
    return N;
}

// dev profile (-DDSA_PB_PROF), thread 0 in front of the commit: cycle sums per phase of the resolving workgroup, read and reset by
// dsa_dbg_pbprof_dump (no printf: it distorts what it measures).  t = {tk0, tk1, tr0, tr1, tr2, tr3}, the stage boundaries of k_plan.
#ifdef DSA_PB_PROF
__device__ __forceinline__ void pbprof_round(const Resolve& S, const Round& R, const Verdict V, const Plan* plans, const long long (&t)[6]) {
    const int G = R.G;
    const long long ph[7] = {t[1] - t[0], t[2] - t[1], t[3] - t[2], t[4] - t[3], t[5] - t[4], (long long)clock64() - t[5], (long long)S.sNConf};
    atomicAdd(&g_pbprof[0], 1ull);
    for (int q = 0; q < 7; ++q) atomicAdd(&g_pbprof[1 + q], (unsigned long long)ph[q]);
    atomicAdd(&g_pbprof[8], (unsigned long long)G); atomicAdd(&g_pbprof[9], (unsigned long long)V.na);
    // why the round ended where it did: 0 the whole window, 10 a BARRIER op (11..17: its reason + 11), 1..9 see the cut sites
    int code = 0;
    if (V.dd < G) code = S.sB <= S.sC ? 11 + (__hip_atomic_load(&plans[S.sB < G ? S.sB : 0].count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 7) : (int)S.sCutWhy[S.sC];
    atomicAdd(&g_pbprof[12 + code], 1ull);
}
#else
__device__ __forceinline__ void pbprof_round(const Resolve&, const Round&, const Verdict, const Plan*, const long long (&)[6]) {}
#endif

// ---- stage 8, commit ---------------------------------------------------------------------------------------------------------------------
// Reads:  the verdict, the next window, the sums of the decide stage, the scalars of the round.
// Writes: thread 0: RoundState (the window of THIS round for k_apply, the description of the next one, the statistics), the Ctl sums,
//         G_next; all threads: PB_DEFER over the action of the deferred ops of [0, dd) — the ops k_apply must skip.
__device__ __forceinline__ void resolve_commit(const Resolve& S, const Round& R, const Verdict V, const NextWindow N, const Ctl* ctl, RoundState* rs,
                                               Plan* plans) {
    const int tid = threadIdx.x, G = R.G, dd = V.dd, na = V.na;
    if (tid == 0) {
        rs->ticket = 0u;                                               // re-armed for the next round
        // commit the window of THIS round (k_apply reads it) ...
        rs->cursor = R.i0; rs->np = R.np; rs->cur = R.cur;
        if (S.sFault) atomicMax(&rs->pad, 9);
        if (G <= 0) { rs->stop = R.drain ? 5 : 2; rs->d = 0; return; }    // finished (5: the pending list is drained)
        rs->ema = V.ema;
        if (V.stop_short) {
            rs->why[S.sB <= S.sC ? (__hip_atomic_load(&plans[S.sB < G ? S.sB : 0].count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 7) : 7] += 1;
            rs->stop = 1; rs->d = 0;
            rs->pend0 = R.op_index(0);
            return;                                                    // (the next window stays what this one was)
        }
        rs->d = dd;
        // ... and describe the next one
        rs->cursor_n = N.cursor_next; rs->np_n = N.np_next; rs->cur_n = 1 - R.cur;
        rs->rounds = R.rounds_prev + (na > 0 ? 1 : 0); rs->par_ops = R.par_ops_prev + na; rs->deferred = R.deferred_prev + S.sNDeferred;
        if (na > 0) {
            Ctl* c = const_cast<Ctl*>(ctl);
            if (S.sSumDn != 0) atomicAdd((unsigned long long*)&c->nb_elements, (unsigned long long)(long long)S.sSumDn);
            if (S.sSumRebN != 0) {
                atomicAdd((unsigned long long*)&c->stat_rebalances, (unsigned long long)S.sSumRebN);
                atomicAdd((unsigned long long*)&c->stat_window_slots, (unsigned long long)S.sSumRebW);
                atomicAdd((unsigned long long*)&c->stat_small_rebalances, (unsigned long long)S.sSumRebN);
            }
        }
        // the next window: half as much again as what ran.  (The resolve step costs per planned op where ops collide: with a floor of 256 /
        // 512 / 1024 ops under the window config 5's first batch takes 50.7 / 58.1 / 68.0 ms instead of 34.0, its first 14 batches 143 / 168 /
        // 192 ms instead of 119; batch B and the matrix updates gain 0-3 % at 1024.)
        int Gn = na + (na >> 1) + 32;
        if (Gn < 64) Gn = 64;
        if (Gn > PB_GMAX) Gn = PB_GMAX;
        rs->G_next = Gn;
    }
    // the ops k_apply must skip: deferred ones inside [0, dd)
    if (!V.stop_short && G > 0 && S.sNDeferred > 0)
        for (int j = tid; j < dd; j += PL_BLOCK)
            if (S.sConf[j] || S.sDefer[j]) __hip_atomic_store(&plans[j].action, (int32_t)PB_DEFER, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
}  // namespace dsa
