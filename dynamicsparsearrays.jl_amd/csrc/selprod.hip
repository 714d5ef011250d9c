// csrc/selprod.hip — K-selprod: the partitions of a key list x dense ROW-MAJOR block of k vectors on gfx950
// (dsa_mat_spmm_selected[_dev]): Y = A[sel, :] X from rowmajor, Y = A[:, sel]' X from colmajor, cost proportional to what is selected.
//
// Y[j, 0:k] = sum over the cells of the live partition whose key is sel[j] of val * X[key - 1, 0:k] (keys 1-based, any order, repeats
// allowed: every occurrence gets its own row).  One wave per selected key, four independent waves per workgroup, no workgroup barrier:
//   span     find_dev.h: key_span — wave-parallel table search, tombstoned entries behind the partition skipped 64 at a time: the
//            cells are the occupied slots of [lo, hi).  Its error is ignored: a key that is < 1, never written or deleted has no live
//            partition and its row is +0.0 (nothing can be reported without a host wait, and this call makes none).
//   load     nine bitmap words at a time (spmm_dev.h: mm_load_compact, SPAN form): occupancy words, keys (physical width) and values,
//            lane <-> slot, coalesced, all requested before anything waits; words behind the span's last word are not fetched anew
//            (the loads are clamped to it); first and last word masked to [lo, hi)
//   compact  the occupied slots go to the wave's LDS slice in slot order (ballot / popcount)
//   walk     KB in {4, 8, 16} lanes, one per column of X, walk the compacted cells IN ORDER (spmm_dev.h: mm_walk), 8 X loads in
//            flight per lane, the adds sequential: one multiply then one add per term (no FMA: -ffp-contract=off), left to right
//            from +0.0 — the order of k_spmm, so a row is bit-identical to the same row of the full product at any length.
// hi is known, so nothing here looks for semaphores.  Every row of Y is stored exactly once with plain stores, zeros included: no
// memset in front of the launch, no atomics, no partial sums.  A long row is walked by its one wave (n / 8 dependent load rounds:
// correct at any length, slow for many thousand cells); a short row leaves 64 - KB lanes idle during the walk.  k > 16 is a loop of
// launches over blocks of 16 columns (the spans are looked up and read once per block).
// Bytes: 8 * nsel keys, about 8 * log2(table_len) probed table bytes per key, (kb + 8 + 1/8) per slot of the selected spans, one
// 64-byte line of X per 8 columns and selected cell, 8 * k * nsel out.  Nothing is proportional to the capacity.
// Measured on config 3 (tools/selprodbench.py, profiles/selprod_c3.json; medians of three runs, k = 1 / 8): 0.1 % of the rows 10.9 /
// 11.1 us, 1 % 26.5 / 26.7 us (the full product + gather: 136 / 226 us, the selected export of the same keys: 93 us), 10 % 195 us,
// 100 % 1.9 ms: the full product is the faster call from somewhere between 1 % and 10 % of the keys at k = 1, between 10 % and 100 %
// at k = 8.  Large selections cost 1.9 ns per key, bound by the wave's chain of dependent loads, not by bytes.  Packing several
// short keys into one wave has not been built or measured.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, int32 keys / int64 keys):
//   94 / 100 VGPRs, 56 / 54 SGPRs, LDS 31 744 / 40 960 B per workgroup (the MmWave slices of k_spmm: 5 / 3 workgroups = 20 / 12
//   waves per CU, which is the limiter), no scratch in any of the 12 instantiations (key width x NT x KB).
#include "selprod.h"
#include "spmm_dev.h"

namespace dsa {

// x, y: first column of the block (the host adds the block's offset); kc <= KB columns of it exist
template <bool WIDE, bool NT, int KB>
__global__ __launch_bounds__(MM_BLOCK) void k_selprod(SlotView V, const int64_t* __restrict__ sel, int64_t nsel,
                                                      const double* __restrict__ x, int64_t nx, int64_t ldx, double* __restrict__ y,
                                                      int64_t ldy, int kc) {
    typedef typename std::conditional<WIDE, int64_t, int32_t>::type key_t;
    __shared__ MmWave<key_t> sW[MM_WAVES];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t j = (int64_t)blockIdx.x * MM_WAVES + wv;
    if (j >= nsel) return;                                   // (whole waves: nothing below waits for another wave)
    const key_t* __restrict__ kp = static_cast<const key_t*>(V.keys.p);
    const double* __restrict__ vals = V.vals;
    const uint64_t* __restrict__ occ = V.occ;
    MmWave<key_t>& S = sW[wv];
    const int col = lane % KB;
    const bool walker = lane < KB;                           // the lanes that sum: one per column
    const bool colok = col < kc;
    const double* __restrict__ xcol = x + (colok ? col : 0);

    // any key may own a live partition (also one beyond size(m)): the table decides
    const KeySpan sp = key_span(V, sel[j], INT64_MAX, lane);
    const int64_t lo = sp.lo, hi = nx > 0 ? sp.hi : sp.lo;   // nx = 0: nothing can contribute (and X may be NULL)
    double sum = 0.0;
    if (hi > lo) {
        const int64_t wend = ((hi - 1) >> 6) + 1;            // words behind the span are not this key's
        for (int64_t w = lo >> 6; w < wend; w += MM_LOAD_WORDS) {
            int none;
            bool closed;
            const int n = mm_load_compact<WIDE, NT, 0, true>(kp, vals, occ, wend, w, nx, S, lane, none, closed, lo, hi);
            __builtin_amdgcn_wave_barrier();
            if (walker) sum = mm_walk<key_t>(sum, 0, n, S, xcol, ldx, colok);
            __builtin_amdgcn_wave_barrier();
        }
    }
    if (walker && colok) y[j * ldy + col] = sum;
}

template <bool WIDE, bool NT>
static void launch_selprod_block(unsigned grid, hipStream_t stream, const SlotView& V, const int64_t* d_sel, int64_t nsel, const double* x,
                                 int64_t nx, int64_t ldx, double* y, int64_t ldy, int kc) {
#define DSA_SELPROD_CASE(KB_) hipLaunchKernelGGL((k_selprod<WIDE, NT, KB_>), dim3(grid), dim3(MM_BLOCK), 0, stream, V, d_sel, nsel, x, nx, \
                                                 ldx, y, ldy, kc)
    if (kc <= 4) DSA_SELPROD_CASE(4);
    else if (kc <= 8) DSA_SELPROD_CASE(8);
    else DSA_SELPROD_CASE(16);
#undef DSA_SELPROD_CASE
}

hipError_t launch_selprod(const SlotView& V, const int64_t* d_sel, int64_t nsel, const double* x, int64_t nx, int64_t k, int64_t ldx,
                          double* y, int64_t ldy, bool nt, hipStream_t stream) {
    if (V.capacity < 0 || V.table_len < 0 || nsel < 0 || nsel > INT32_MAX) return hipErrorInvalidValue;
    if (nsel == 0 || k <= 0) return hipSuccess;
    const unsigned grid = (unsigned)((nsel + MM_WAVES - 1) / MM_WAVES);
    for (int64_t jb = 0; jb < k; jb += 16) {
        const int kc = (int)(k - jb < 16 ? k - jb : 16);
        const int which = (V.keys.wide ? 2 : 0) | (nt ? 1 : 0);
#define DSA_SELPROD_BLOCK(W_, N_) launch_selprod_block<W_, N_>(grid, stream, V, d_sel, nsel, x + jb, nx, ldx, y + jb, ldy, kc)
        switch (which) {
            case 0: DSA_SELPROD_BLOCK(false, false); break;
            case 1: DSA_SELPROD_BLOCK(false, true); break;
            case 2: DSA_SELPROD_BLOCK(true, false); break;
            default: DSA_SELPROD_BLOCK(true, true); break;
        }
#undef DSA_SELPROD_BLOCK
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace dsa
