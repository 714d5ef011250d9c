// csrc/pb_fpcheck.h — footprint-check build of the batch-parallel writes (-DDSA_FP_CHECK; make libdsa_hip_fpcheck.so).  Included by
// parbatch.hip alone, behind its constants and the helpers that decode a Plan.  The production kernels call the hooks below where the
// check needs something from them; in the default build every hook is empty and the kernels compile as if the calls were not there.
#pragma once

namespace dsa {
// The resolve step lets ops run side by side on the strength of their DECLARED footprints.  Three footprint-class defects hid behind green
// suites for two rounds (Oracle and parity); this build makes the soundness of a round mechanical instead of argued:
//   mode 1 (recorded sets)  the plan records what it literally scanned for its shift target (the occupancy runs of _nextemptypos /
//            _previousemptypos) and every window whose cell count it consulted; the apply records the hull of every slot it wrote or
//            re-read live.  k_fp_pre then re-derives the resolver's verdict by BRUTE FORCE, without its spatial hash: the final footprints of
//            the prefix are pairwise disjoint, every scanned run lies inside the op's footprint, every counted window either lies inside it
//            (and no other op of the prefix changes a bit there) or is the leaf of a leaf-accepted op whose thresholds hold for the count
//            recounted from the bitmap plus / minus ALL changes the prefix makes in that leaf.  k_fp_post: what the apply touched lies inside
//            the footprint.
//   mode 2 (sequential shadow)  the prefix is applied one op after the other by ONE wave; before each op its plan is recomputed on the
//            LIVE state and must equal the plan the round was resolved on (action, positions, accepted window, count when a rebalance
//            follows): "each op sees exactly the state it was planned on", checked, for every semantic dependency at once (also the ones
//            of the 64-ary find, whose literal probes are far outside any footprint).
// A violation prints its details and raises RoundState::pad (the host fails the batch).  DSA_FP_REGRESS=1 / 2 re-introduce the two
// resolver bugs of round 4 (the leaf walk of ONE hash cell; the footprint of a left-falling insert ending at p + 1), = 3 the one this build
// found itself (a widened new column whose window ends on a hash-cell boundary is not chained in the next cell): the check must fire.
// The checker is the reference the resolver is tested against: it shares nothing with the resolver's hash, tallies or widening.
#ifndef DSA_FP_REGRESS
#define DSA_FP_REGRESS 0
#endif

#ifdef DSA_FP_CHECK
// what the check re-runs (parbatch.hip)
__device__ Plan pb_plan_one(KeyArr keys, const double* vals, const uint64_t* occ, const int64_t* sems, const int64_t* col_keys,
                            const uint8_t* col_live, const Ctl* ctl, const Op op, int w, int max_w);
__device__ void pb_apply_one(KeyArr keys, double* vals, uint64_t* occ, int64_t* sems, int64_t* col_keys, uint8_t* col_live, Ctl* ctl,
                             int32_t* fault, const Op op, const Plan pl, int64_t* sK, double* sV, const bool counted);

constexpr int FP_MAXCNT = 12;
struct FpRec {                                    // what ONE op of a round literally read (plan) and touched (apply)
    int64_t rlo, rhi;                             // occupancy runs scanned for the shift target (1-based, inclusive; rlo > rhi: none)
    int64_t tlo, thi;                             // slots written, bits changed, cells re-read live by the apply
    int32_t ncnt, pad;
    int32_t cnt[FP_MAXCNT][2];                    // windows whose cell count the plan consulted
};
struct FpIv { int32_t lo, hi; };                  // the FINAL footprint the resolve step used (after widening)
static_assert(sizeof(FpRec) + sizeof(FpIv) <= FP_BYTES_PER_OP, "the host sizes the plan array for the records behind it");
__shared__ FpRec g_fpw[16];                       // one recorder per wave of the workgroup (k_plan: 16, k_apply: 4, k_local_rounds: 8)
__shared__ FpRec g_fplan[8];                      // k_local_rounds: what the wave's plan recorded, kept across the apply (which resets the recorder)
// the records behind the plans of a round: one FpRec per op, then one FpIv per op
__device__ __forceinline__ FpRec* fp_recs(const Plan* plans) { return reinterpret_cast<FpRec*>(const_cast<Plan*>(plans) + PB_GMAX); }
__device__ __forceinline__ FpIv* fp_ivs(const Plan* plans) { return reinterpret_cast<FpIv*>(fp_recs(plans) + PB_GMAX); }

// ---- recorders (pb_plan_one, pb_apply_one and what they call) ------------------------------------------------------------------------
__device__ __forceinline__ void fp_reset() {
    if (lane_id() == 0) { FpRec& f = g_fpw[threadIdx.x >> 6]; f.rlo = INT64_MAX; f.rhi = 0; f.tlo = INT64_MAX; f.thi = 0; f.ncnt = 0; f.pad = 0; }
}
__device__ __forceinline__ void fp_pos(int64_t a, int64_t b) {
    if (lane_id() == 0 && a <= b) { FpRec& f = g_fpw[threadIdx.x >> 6]; if (a < f.rlo) f.rlo = a; if (b > f.rhi) f.rhi = b; }
}
__device__ __forceinline__ void fp_touch(int64_t a, int64_t b) {
    if (lane_id() == 0 && a <= b) { FpRec& f = g_fpw[threadIdx.x >> 6]; if (a < f.tlo) f.tlo = a; if (b > f.thi) f.thi = b; }
}
__device__ __forceinline__ void fp_cnt(int64_t a, int64_t b) {
    if (lane_id() == 0) {
        FpRec& f = g_fpw[threadIdx.x >> 6];
        if (f.ncnt < FP_MAXCNT) { f.cnt[f.ncnt][0] = (int32_t)a; f.cnt[f.ncnt][1] = (int32_t)b; }
        f.ncnt += 1;
    }
}

// ---- hooks of k_plan and k_apply ---------------------------------------------------------------------------------------------------------
// k_plan, behind the plan of op w: its record, read by k_fp_pre, the next kernel of the round
__device__ __forceinline__ void fp_publish_plan(Plan* plans, int w) {
    __builtin_amdgcn_wave_barrier();
    if (lane_id() == 0) fp_recs(plans)[w] = g_fpw[threadIdx.x >> 6];
}
// resolve step, behind the seal stage: the final footprints, for the brute-force re-derivation of this verdict (k_fp_pre)
template <class IV>
__device__ __forceinline__ void fp_publish_footprints(Plan* plans, const IV* iv, int n) {
    FpIv* fiv = fp_ivs(plans);
    for (int j = threadIdx.x; j < n; j += blockDim.x) { fiv[j].lo = iv[j].lo; fiv[j].hi = iv[j].hi; }
}
// seal stage (dev knob: bit 0x400 of RoundState::tight): an op that was sealed
__device__ __forceinline__ void fp_note_sealed(const RoundState* rs, long long op, int j, int act, int lo, int hi, long long A, long long B, long long W) {
    if (rs->tight & 0x400) printf("DSA_FP_CHECK run-ahead: op %lld (position %d, act %d, footprint [%d,%d]) sealed in [%lld,%lld]+[..%lld]\n", op, j, act, lo, hi, A, B, B + W);
}
// decide stage: a pending op that left the zone it was sealed in
__device__ __forceinline__ void fp_note_zone_fault(const PendOp& po, int j, int np, int lo, int hi, int act) {
    printf("DSA_FP_CHECK run-ahead: pending op %lld (window position %d of %d pending) is applied with the footprint [%d,%d] (act %d), outside the zone [%d,%d] it was sealed in\n",
           (long long)po.op, j, np, lo, hi, act, po.zlo, po.zhi);
}
// k_apply, mode 2: the prefix was applied one op after the other by k_fp_pre
__device__ __forceinline__ bool fp_shadow_applied(const RoundState* rs) { return (rs->tight & FP_MODE_SHADOW) != 0; }
// k_apply, behind the apply of op w: what it touched, read by k_fp_post
__device__ __forceinline__ void fp_publish_touched(const Plan* plans, int w) {
    __builtin_amdgcn_wave_barrier();
    if (lane_id() == 0) {
        FpRec* rec = fp_recs(plans) + w;
        const FpRec& f = g_fpw[threadIdx.x >> 6];
        rec->tlo = f.tlo; rec->thi = f.thi;
    }
}

// do two plans of one op describe the same effect?  (footprints and the leaf counts carried for the resolver may differ)
__device__ bool fp_same_plan(const Plan& a, const Plan& b, int64_t seg) {
    if (a.action != b.action) return false;
    switch (a.action) {
        case PB_NOOP: case PB_BARRIER: return true;
        case PB_OVERWRITE: return a.pos == b.pos;
        case PB_NEWCOL: {
            if (a.pos != b.pos || a.aux != b.aux) return false;
            const bool ta = (a.count & 0x80) != 0, tb = (b.count & 0x80) != 0;
            if (ta && tb) return a.hi == b.hi;                                      // both leaf-accepted: the same two gaps
            return ta == tb && a.ws == b.ws && a.we == b.we && (a.count & 0x7f) == (b.count & 0x7f);
        }
        default:
            if (a.pos != b.pos || a.aux != b.aux || a.ws != b.ws || a.we != b.we) return false;
            return (a.we - a.ws + 1 == seg) || a.count == b.count;                  // a rebalance follows: it spreads `count` cells
    }
}
__device__ __forceinline__ void fp_fault(RoundState* rs, int code) { atomicMax(&rs->pad, code); }

// Between k_plan (+ resolve) and k_apply.  Mode 1: the brute-force re-derivation described at the top of this file.  Mode 2: the
// sequential shadow — wave 0 re-plans every op of the prefix on the live state, compares, applies it.
__global__ __launch_bounds__(PL_BLOCK) void k_fp_pre(const DevBufs* bufs, Ctl* ctl, const Op* ops, RoundState* rs, Plan* plans) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pb_lds[];
    if (rs->stop) return;
    const int d = rs->d;
    if (d <= 0) return;
    const int mode = rs->tight;
    const DevBufs db = *bufs;
    const KeyArr keys{db.keys, db.wide, 0};
    double* vals = db.vals; uint64_t* occ = db.occ;
    int64_t* sems = db.sems; int64_t* col_keys = db.col_keys; uint8_t* col_live = db.col_live;
    const int64_t i0 = rs->cursor, seg = ctl->segment_capacity;
    const int tid = threadIdx.x;
    if (mode & FP_MODE_SHADOW) {
        if (tid >= 64) return;
        int64_t* sK = reinterpret_cast<int64_t*>(pb_lds);
        double* sV = reinterpret_cast<double*>(pb_lds + (size_t)PB_MAX_W * sizeof(int64_t));
        const int np = rs->np;
        const PendOp* pend = db.pend + (size_t)rs->cur * PB_GMAX;
        for (int j = 0; j < d; ++j) {
            const Plan want = plans[j];
            if (want.action == PB_DEFER) continue;                  // deferred: not part of this round
            const Op op = ops[j < np ? pend[j].op : i0 + (j - np)];
            // (w = 0: the table entries of the earlier new columns exist by now)
            const Plan live = pb_plan_one(keys, vals, occ, sems, col_keys, col_live, ctl, op, 0, PB_MAX_W);
            if (!fp_same_plan(want, live, seg)) {
                if (tid == 0) {
                    printf("DSA_FP_CHECK shadow: op %lld (round op %d of %d; a %lld b %lld v %g) planned act %d pos %lld aux %lld win [%lld,%lld] count %d fp [%lld,%lld]"
                           " | on the state left by the earlier ops of its round: act %d pos %lld aux %lld win [%lld,%lld] count %d fp [%lld,%lld]\n",
                           (long long)(i0 + j), j, d, (long long)op.a, (long long)op.b, op.v, want.action, (long long)want.pos, (long long)want.aux,
                           (long long)want.ws, (long long)want.we, want.count, (long long)want.lo, (long long)want.hi, live.action, (long long)live.pos,
                           (long long)live.aux, (long long)live.ws, (long long)live.we, live.count, (long long)live.lo, (long long)live.hi);
                    fp_fault(rs, 12);
                }
                return;                                              // nothing more is applied: the host fails the batch
            }
            pb_apply_one(keys, vals, occ, sems, col_keys, col_live, ctl, &rs->pad, op, want, sK, sV, true);
            __builtin_amdgcn_s_waitcnt(0);                           // this wave's stores and atomics have been acknowledged (they are at the L2) ...
            __builtin_amdgcn_s_dcache_inv();                         // ... and the next plan reads neither through a stale scalar cache
            asm volatile("buffer_inv sc0" ::: "memory");            // nor through this CU's vector L1
        }
        return;
    }
    if (!(mode & FP_MODE_SETS)) return;
    const FpRec* recs = fp_recs(plans);
    const FpIv* fiv = fp_ivs(plans);
    __shared__ int32_t sLo[PB_GMAX], sHi[PB_GMAX], sC1[PB_GMAX], sC2[PB_GMAX], sWs[PB_GMAX], sWe[PB_GMAX], sTLo[PB_GMAX], sTHi[PB_GMAX];
    __shared__ signed char sD1[PB_GMAX];
    __shared__ unsigned char sTight[PB_GMAX];
    __shared__ unsigned char sOff[PB_GMAX];                          // deferred by the resolve step: not part of this round
    for (int j = tid; j < d; j += PL_BLOCK) {
        const Plan q = plans[j];
        sOff[j] = q.action == PB_DEFER ? 1 : 0;
        const bool leaf_only = pb_is_leaf_only(q.action, q.ws, q.we, seg, q.count);
        const int dl = pb_delta(q.action, leaf_only);
        sLo[j] = fiv[j].lo; sHi[j] = fiv[j].hi;
        if (sOff[j]) { sLo[j] = INT32_MAX; sHi[j] = INT32_MIN; }
        sD1[j] = (signed char)dl;
        sC1[j] = dl != 0 ? (int32_t)pb_changed_slot(q.action, q.pos, q.aux) : 0;
        sC2[j] = (q.action == PB_NEWCOL && leaf_only) ? (int32_t)q.hi : 0;
        // an op that rebalances (or a new column that may) changes any bit of its window
        const bool reb = (q.action == PB_NEWCOL && !leaf_only) ||
                         ((q.action == PB_INS_R || q.action == PB_INS_L || q.action == PB_DELETE) && q.we - q.ws + 1 != seg);
        sWs[j] = reb ? (int32_t)q.ws : 1; sWe[j] = reb ? (int32_t)q.we : 0;
        sTight[j] = leaf_only ? 1 : 0;
        // what the apply may WRITE or re-read live: a leaf-accepted insert / delete moves nothing but its shifted run — its tight hull,
        // also when the resolve step widened the footprint to the leaf (the widening stands for the COUNT the plan read) —, everybody
        // else anything inside the final footprint (a new column that was widened scans and rebalances live inside its window)
        const bool hull_only = leaf_only && q.action != PB_NEWCOL;
        sTLo[j] = hull_only ? (int32_t)q.lo : fiv[j].lo; sTHi[j] = hull_only ? (int32_t)q.hi : fiv[j].hi;
        if (sOff[j]) { sTLo[j] = INT32_MAX; sTHi[j] = INT32_MIN; }
    }
    __syncthreads();
    const int64_t lo0 = ctl->lo[0], hi0 = ctl->hi[0];
    for (int j = tid; j < d; j += PL_BLOCK) {
        if (sOff[j]) continue;
        const int32_t lo = sLo[j], hi = sHi[j];
        const FpRec r = recs[j];
        // (a) nothing an EARLIER op of the prefix writes lies in the final footprint of a later one (which holds everything that one read for
        //     its decisions and everything it writes) — all pairs, no hash.  The converse — a later op writing where an earlier one only
        //     COUNTED — is allowed: the earlier plan was made on the pre-round state either way, as the sequential order has it.
        if (lo <= hi)
            for (int i = 0; i < j; ++i)
                if (sTLo[i] <= sTHi[i] && sTLo[i] <= hi && lo <= sTHi[i]) {
                    printf("DSA_FP_CHECK sets: op %d of a prefix of %d writes inside [%d,%d] (footprint [%d,%d]); the later op %d has the footprint [%d,%d]\n", i, d,
                           sTLo[i], sTHi[i], sLo[i], sHi[i], j, lo, hi);
                    fp_fault(rs, 13);
                }
        if (sTLo[j] < lo || sTHi[j] > hi) { printf("DSA_FP_CHECK sets: op %d: write set [%d,%d] outside its footprint [%d,%d]\n", j, sTLo[j], sTHi[j], lo, hi); fp_fault(rs, 13); }
        // (b) the occupancy runs the plan scanned for its shift target lie inside the footprint
        if (r.rlo <= r.rhi && (r.rlo < lo || r.rhi > hi)) {
            printf("DSA_FP_CHECK sets: op %d (act %d) scanned the occupancy of [%lld,%lld] for its shift target, its footprint is [%d,%d]\n", j, plans[j].action,
                   (long long)r.rlo, (long long)r.rhi, lo, hi);
            fp_fault(rs, 14);
        }
        // (c) every window whose count the plan consulted: inside the footprint and untouched by the others, or the leaf of a leaf-accepted
        //     op whose thresholds hold whatever subset of the prefix's changes has happened
        if (r.ncnt > FP_MAXCNT) { printf("DSA_FP_CHECK sets: op %d consulted %d windows (recorder holds %d)\n", j, r.ncnt, FP_MAXCNT); fp_fault(rs, 15); }
        for (int c = 0; c < r.ncnt && c < FP_MAXCNT; ++c) {
            const int32_t a = r.cnt[c][0], b = r.cnt[c][1];
            const bool inside = a >= lo && b <= hi;
            int ins = 0, del = 0, foreign = 0;
            for (int i = 0; i < d; ++i) {
                if (i != j && sWs[i] <= sWe[i] && sWs[i] <= b && a <= sWe[i]) ++foreign;       // somebody else's rebalance window reaches in
                const int32_t c1 = sC1[i], c2 = sC2[i];
                if (c1 >= a && c1 <= b) { if (sD1[i] > 0) ++ins; else ++del; if (i != j && inside) ++foreign; }
                if (c2 >= a && c2 <= b) { ++ins; if (i != j && inside) ++foreign; }
            }
            if (inside) {
                if (foreign) { printf("DSA_FP_CHECK sets: op %d counted [%d,%d] inside its footprint [%d,%d]; %d other ops of the prefix change it\n", j, a, b, lo, hi, foreign); fp_fault(rs, 16); }
                continue;
            }
            if (sTight[j] && plans[j].action == PB_NEWCOL && b - a + 1 != seg) continue;      // the fallback window of a leaf-accepted new column: only consulted if the resolve step widens the op to it — then it is inside
            if (!sTight[j] || b - a + 1 != seg) {
                printf("DSA_FP_CHECK sets: op %d (act %d) counted [%d,%d] outside its footprint [%d,%d] and is not leaf-accepted\n", j, plans[j].action, a, b, lo, hi);
                fp_fault(rs, 17);
                continue;
            }
            if (foreign) { printf("DSA_FP_CHECK sets: leaf [%d,%d] of op %d lies in another op's rebalance window\n", a, b, j); fp_fault(rs, 18); continue; }
            int64_t cnt = 0;                                                   // recounted from the pre-round bitmap
            for (int64_t w = (a - 1) >> 6; w <= (b - 1) >> 6; ++w) cnt += popc64(occ[w] & word_range_mask(w, a - 1, b - 1));
            if (!(cnt + ins <= hi0 && cnt - del >= lo0)) {
                printf("DSA_FP_CHECK sets: leaf [%d,%d] of leaf-accepted op %d (act %d, footprint [%d,%d]) holds %lld cells; the prefix of %d ops inserts %d and deletes %d "
                       "there: thresholds [%lld,%lld] do not hold for every order\n", a, b, j, plans[j].action, lo, hi, (long long)cnt, d, ins, del, (long long)lo0, (long long)hi0);
                fp_fault(rs, 19);
            }
        }
    }
}
// behind k_apply (mode 1): what every op of the prefix wrote, changed or re-read live lies inside its final footprint
__global__ __launch_bounds__(PL_BLOCK) void k_fp_post(RoundState* rs, const Plan* plans, const Ctl* ctl) {
    if (rs->stop || !(rs->tight & FP_MODE_SETS) || (rs->tight & FP_MODE_SHADOW)) return;
    const int d = rs->d;
    const int64_t seg = ctl->segment_capacity;
    const FpRec* recs = fp_recs(plans);
    const FpIv* fiv = fp_ivs(plans);
    for (int j = threadIdx.x; j < d; j += PL_BLOCK) {
        const FpRec r = recs[j];
        const Plan q = plans[j];
        if (q.action == PB_DEFER) continue;
        const bool hull_only = q.action != PB_NEWCOL && pb_is_leaf_only(q.action, q.ws, q.we, seg, q.count);      // (see k_fp_pre)
        const int64_t tlo = hull_only ? q.lo : (int64_t)fiv[j].lo, thi = hull_only ? q.hi : (int64_t)fiv[j].hi;
        if (r.tlo <= r.thi && (r.tlo < tlo || r.thi > thi)) {
            printf("DSA_FP_CHECK sets: op %d (act %d) touched [%lld,%lld], it may write [%lld,%lld] (footprint [%d,%d])\n", j, q.action, (long long)r.tlo, (long long)r.thi,
                   (long long)tlo, (long long)thi, fiv[j].lo, fiv[j].hi);
            fp_fault(rs, 20);
        }
    }
}
// enqueue_round: the two check kernels around k_apply
inline void fp_enqueue_pre(const DevBufs* bufs, Ctl* ctl, const Op* ops, RoundState* rs, Plan* plans, hipStream_t stream) {
    hipLaunchKernelGGL(k_fp_pre, dim3(1), dim3(PL_BLOCK), PB_WAVE_LDS, stream, bufs, ctl, ops, rs, plans);
}
inline void fp_enqueue_post(RoundState* rs, const Plan* plans, const Ctl* ctl, hipStream_t stream) {
    hipLaunchKernelGGL(k_fp_post, dim3(1), dim3(PL_BLOCK), 0, stream, rs, plans, ctl);
}

// ---- hooks of k_local_rounds (dd: the prefix of the mini-round, sPlan: its plans, one wave per op) ------------------------------------
// Mode 2, the sequential shadow of the mini-round: op j is planned again on the state the ops before it left, compared, applied.
// Returns true when it has applied the prefix in the kernel's stead.
__device__ __forceinline__ bool fp_lr_shadow(KeyArr keys, double* vals, uint64_t* occ, int64_t* sems, int64_t* col_keys, uint8_t* col_live, Ctl* ctl,
                                             const Op* ops, RoundState* rs, const Plan* sPlan, int dd, int64_t cursor, int max_w, int64_t* sK, double* sV) {
    if (!(rs->tight & FP_MODE_SHADOW)) return false;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int j = 0; j < dd; ++j) {
        if (wv == j) {
            const Op op = ops[cursor + j];
            const Plan live = pb_plan_one(keys, vals, occ, sems, col_keys, col_live, ctl, op, 0, max_w);
            if (!fp_same_plan(sPlan[j], live, ctl->segment_capacity)) {
                if (lane == 0) {
                    printf("DSA_FP_CHECK shadow (local rounds): op %lld (%d of %d) planned act %d pos %lld aux %lld win [%lld,%lld] | live act %d pos %lld aux %lld win [%lld,%lld]\n",
                           (long long)(cursor + j), j, dd, sPlan[j].action, (long long)sPlan[j].pos, (long long)sPlan[j].aux, (long long)sPlan[j].ws, (long long)sPlan[j].we,
                           live.action, (long long)live.pos, (long long)live.aux, (long long)live.ws, (long long)live.we);
                    fp_fault(rs, 22);
                }
            } else pb_apply_one(keys, vals, occ, sems, col_keys, col_live, ctl, &rs->pad, op, sPlan[j], sK, sV, false);
        }
        __builtin_amdgcn_s_waitcnt(0);
        __syncthreads();
        __builtin_amdgcn_s_dcache_inv();
        asm volatile("buffer_inv sc0" ::: "memory");
    }
    return true;
}
// Mode 1, in front of the apply: what the wave's plan recorded is put aside
__device__ __forceinline__ void fp_lr_keep_plan_record(int dd) {
    const int wv = threadIdx.x >> 6;
    if (wv < dd && lane_id() == 0) g_fplan[wv] = g_fpw[wv];
}
// Mode 1, behind the apply — recorded sets: the run the plan scanned and what the apply touched lie inside the op's FULL footprint (what
// the kernel's all-pairs test works on), and those are pairwise disjoint
template <int WAVES>
__device__ __forceinline__ void fp_lr_check_sets(RoundState* rs, const Ctl* ctl, const Plan* sPlan, int dd) {
    static_assert(WAVES <= (int)(sizeof(g_fplan) / sizeof(g_fplan[0])), "one kept record per wave");
    const int wv = threadIdx.x >> 6;
    __builtin_amdgcn_wave_barrier();
    if (wv < dd && lane_id() == 0) { g_fplan[wv].tlo = g_fpw[wv].tlo; g_fplan[wv].thi = g_fpw[wv].thi; }
    __syncthreads();
    if ((rs->tight & FP_MODE_SETS) && threadIdx.x == 0) {
        const int64_t segc = ctl->segment_capacity;
        int64_t flo[WAVES], fhi[WAVES];
        for (int j = 0; j < dd; ++j) {
            const Plan& q = sPlan[j];
            pb_full_footprint(q, segc, ctl->capacity, flo[j], fhi[j]);
            for (int i = 0; i < j; ++i)
                if (flo[i] <= fhi[i] && flo[j] <= fhi[j] && flo[i] <= fhi[j] && flo[j] <= fhi[i]) { printf("DSA_FP_CHECK sets (local rounds): ops %d and %d share slots\n", i, j); fp_fault(rs, 23); }
            const FpRec& r = g_fplan[j];
            if ((r.rlo <= r.rhi && (r.rlo < flo[j] || r.rhi > fhi[j])) || (r.tlo <= r.thi && (r.tlo < flo[j] || r.thi > fhi[j]))) {
                printf("DSA_FP_CHECK sets (local rounds): op %d (act %d) scanned [%lld,%lld] touched [%lld,%lld], footprint [%lld,%lld]\n", j, q.action,
                       (long long)r.rlo, (long long)r.rhi, (long long)r.tlo, (long long)r.thi, (long long)flo[j], (long long)fhi[j]);
                fp_fault(rs, 24);
            }
            for (int c = 0; c < r.ncnt && c < FP_MAXCNT; ++c)
                if (r.cnt[c][0] < flo[j] || r.cnt[c][1] > fhi[j]) { printf("DSA_FP_CHECK sets (local rounds): op %d counted [%d,%d] outside [%lld,%lld]\n", j, r.cnt[c][0], r.cnt[c][1], (long long)flo[j], (long long)fhi[j]); fp_fault(rs, 25); }
        }
    }
}
#else
// the default build: every hook is empty
__device__ __forceinline__ void fp_reset() {}
__device__ __forceinline__ void fp_pos(int64_t, int64_t) {}
__device__ __forceinline__ void fp_touch(int64_t, int64_t) {}
__device__ __forceinline__ void fp_cnt(int64_t, int64_t) {}
__device__ __forceinline__ void fp_publish_plan(Plan*, int) {}
template <class IV> __device__ __forceinline__ void fp_publish_footprints(Plan*, const IV*, int) {}
template <class... A> __device__ __forceinline__ void fp_note_sealed(A...) {}
template <class... A> __device__ __forceinline__ void fp_note_zone_fault(A...) {}
__device__ __forceinline__ bool fp_shadow_applied(const RoundState*) { return false; }
__device__ __forceinline__ void fp_publish_touched(const Plan*, int) {}
template <class... A> __device__ __forceinline__ bool fp_lr_shadow(A...) { return false; }
__device__ __forceinline__ void fp_lr_keep_plan_record(int) {}
template <int WAVES> __device__ __forceinline__ void fp_lr_check_sets(RoundState*, const Ctl*, const Plan*, int) {}
inline void fp_enqueue_pre(const DevBufs*, Ctl*, const Op*, RoundState*, Plan*, hipStream_t) {}
inline void fp_enqueue_post(RoundState*, const Plan*, const Ctl*, hipStream_t) {}
#endif
}  // namespace dsa
