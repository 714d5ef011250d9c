// csrc/spmm.hip — K-spmm: PCSR sparse matrix x dense ROW-MAJOR block of k vectors on gfx950 (dsa_mat_spmm_dense[_dev]).
//
// Y[part_key(p), 0:k] = sum over the cells of partition p of val * X[key, 0:k] — the k-column form of _mul (src/operations.jl:107-135)
// over the twin orientation, like the gather form of spmv.hip.  A cell needs k CONSECUTIVE doubles of X: at k = 8 one 64-byte line,
// all of it used (the single product fetches a line to use 8 bytes of it once x outgrows an XCD's L2), and the slot stream is read
// once for up to 16 columns instead of once per column.  Nothing of the column-swept plan is used.
//
// One wave per span of 512 slots (8 occupancy words), four independent waves per workgroup, no workgroup barrier (load / compact and
// walk are mm_load_compact and mm_walk of spmm_dev.h, shared with selprod.hip):
//   load     occupancy words, keys (physical width) and values of the span and of the word behind it, lane <-> slot, coalesced, all
//            requested before anything waits;
//   compact  the occupied slots go to the wave's LDS slice in slot order (ballot / popcount): 0-based X row (-1: key outside 1..nx)
//            and value; the positions of the span's semaphores are listed apart;
//   walk     lane = (row group lane / KB, column lane % KB): 64 / KB rows are summed at once, each by KB lanes that walk the row's
//            cells IN ORDER, 8 X loads in flight per lane, the adds sequential: one multiply then one add per term (no FMA:
//            -ffp-contract=off), left to right from +0.0 — the reference's order (src/operations.jl:101) for EVERY row.
// Ownership: a row belongs to the wave whose span holds its semaphore.  The owner walks on behind its span — 9 words at a time,
// loaded and compacted by the whole wave, summed by the owning lane group — until the next semaphore or the end of the array; the
// cells in front of a wave's first semaphore belong to an earlier wave and are skipped.  Every Y row is stored exactly once with
// plain stores: no atomics, no partial sums, so there is NO length limit L behind which a row would leave the reference order (a
// row of n cells costs its owner n / 8 dependent load rounds: correct at any length, slow for rows of many thousand cells).
// Rows without a partition are zeroed by the host in front of the launch.  Tombstones, tables out of key order and pending table
// entries need nothing special: the partition id is the semaphore's stored value, its key part_keys[id - 1] (as in k_spmv_gather).
//
// Columns: KB in {4, 8, 16} lanes per row, the block's tail predicated (kc <= KB).  k > 16 is a loop of launches over blocks of 16
// columns: the slot stream is re-read once per block.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, int32 keys / int64 keys):
//   LDS 31 744 / 40 960 B per workgroup (per wave 576 x 8 B values + 576 x 4 | 8 B rows + 512 x 2 B semaphore list): 5 / 3 workgroups
//   = 20 / 12 waves per CU, which is the limiter; 62 VGPRs, 80 SGPRs, no scratch in every instantiation.
#include "spmm.h"
#include "spmm_dev.h"

namespace dsa {

// x, y: first column of the block (the host adds the block's offset); kc <= KB columns of it exist
template <bool WIDE, bool NT, int KB>
__global__ __launch_bounds__(MM_BLOCK) void k_spmm(KeyArr keys, const double* __restrict__ vals, const uint64_t* __restrict__ occ,
                                                   int64_t capacity, const int64_t* __restrict__ part_keys, int64_t table_len,
                                                   const double* __restrict__ x, int64_t nx, int64_t ldx, double* __restrict__ y,
                                                   int64_t ny, int64_t ldy, int kc) {
    typedef typename std::conditional<WIDE, int64_t, int32_t>::type key_t;
    __shared__ MmWave<key_t> sW[MM_WAVES];
    // XCD-aware tile mapping (see k_spmv_gather): XCD g streams the g-th contiguous eighth of the slot array, so the word behind a
    // span and the spans an owner walks on into are lines its own L2 is fetching anyway
    const int64_t ntiles = (capacity + MM_TILE - 1) / MM_TILE;
    int64_t tile = blockIdx.x;
    if (ntiles >= 64) {
        const int64_t per = (ntiles + 7) / 8;
        tile = (int64_t)(blockIdx.x & 7) * per + (blockIdx.x >> 3);
        if (tile >= ntiles) return;
    }
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t nwords = (capacity + 63) >> 6;          // slot buffers are allocated in whole words
    const int64_t w0 = tile * (MM_TILE / 64) + (int64_t)wv * MM_OWN_WORDS;
    if (w0 >= nwords) return;                             // (whole waves: nothing below waits for another wave)
    const key_t* __restrict__ kp = static_cast<const key_t*>(keys.p);
    MmWave<key_t>& S = sW[wv];
    constexpr int G = 64 / KB;
    const int grp = lane / KB, j = lane % KB;
    const bool colok = j < kc;
    const double* __restrict__ xcol = x + (colok ? j : 0);
    double* __restrict__ ycol = y + j;

    int nsem;
    bool closed;
    int n = mm_load_compact<WIDE, NT, MM_OWN_WORDS>(kp, vals, occ, nwords, w0, nx, S, lane, nsem, closed);
    if (nsem == 0) return;                                // every cell of the span belongs to an earlier wave's row
    if (w0 + MM_LOAD_WORDS >= nwords) closed = true;      // nothing behind what was loaded
    __builtin_amdgcn_wave_barrier();

    const int last = nsem - 1;
    double open_sum = 0.0;                                // the span's last row while it is open (owner group only)
    int64_t open_row = 0;
    for (int e = grp; e < nsem; e += G) {
        const int a = S.sem[e];
        const int end = e == last ? n : (int)S.sem[e + 1];
        const int64_t id = (int64_t)S.v[a];              // partition ids are stored as Float64 (src/pcsr.jl:104)
        int64_t row = 0;
        if (id >= 1 && id <= table_len) row = part_keys[id - 1];
        const double sum = mm_walk<key_t>(0.0, a + 1, end, S, xcol, ldx, colok);
        if (e == last && !closed) { open_sum = sum; open_row = row; }
        else if (colok && row >= 1 && row <= ny) ycol[(row - 1) * ldy] = sum;
    }
    if (closed) return;
    // ---- the last row runs on behind the loaded words: the wave loads and compacts, the owning group keeps adding -----------------
    const int owner = last % G;
    for (int64_t w = w0 + MM_LOAD_WORDS; !closed; ) {
        __builtin_amdgcn_wave_barrier();
        int none;
        n = mm_load_compact<WIDE, NT, 0>(kp, vals, occ, nwords, w, nx, S, lane, none, closed);
        w += MM_LOAD_WORDS;
        if (w >= nwords) closed = true;
        __builtin_amdgcn_wave_barrier();
        if (grp == owner) open_sum = mm_walk<key_t>(open_sum, 0, n, S, xcol, ldx, colok);
    }
    if (grp == owner && colok && open_row >= 1 && open_row <= ny) ycol[(open_row - 1) * ldy] = open_sum;
}

template <bool WIDE, bool NT>
static void launch_spmm_block(unsigned grid, hipStream_t stream, const SlotView& V, const double* x, int64_t nx, int64_t ldx, double* y,
                              int64_t ny, int64_t ldy, int kc) {
#define DSA_SPMM_CASE(KB_) hipLaunchKernelGGL((k_spmm<WIDE, NT, KB_>), dim3(grid), dim3(MM_BLOCK), 0, stream, V.keys, V.vals, V.occ, V.capacity, \
                                              V.part_keys, V.table_len, x, nx, ldx, y, ny, ldy, kc)
    if (kc <= 4) DSA_SPMM_CASE(4);
    else if (kc <= 8) DSA_SPMM_CASE(8);
    else DSA_SPMM_CASE(16);
#undef DSA_SPMM_CASE
}

// Y[:, 0:k] = P X[:, 0:k]; Y is NOT zeroed here (rows without a partition keep what they hold).  nt: non-temporal slot loads.
hipError_t launch_spmm(const SlotView& V, const double* x, int64_t nx, int64_t k, int64_t ldx, double* y, int64_t ny, int64_t ldy, bool nt,
                       hipStream_t stream) {
    if (V.capacity <= 0 || k <= 0) return hipSuccess;
    const int64_t ntiles = (V.capacity + MM_TILE - 1) / MM_TILE;
    const unsigned grid = (unsigned)(ntiles >= 64 ? 8 * ((ntiles + 7) / 8) : ntiles);
    for (int64_t jb = 0; jb < k; jb += 16) {
        const int kc = (int)(k - jb < 16 ? k - jb : 16);
        const int sel = (V.keys.wide ? 2 : 0) | (nt ? 1 : 0);
#define DSA_SPMM_BLOCK(W_, N_) launch_spmm_block<W_, N_>(grid, stream, V, x + jb, nx, ldx, y + jb, ny, ldy, kc)
        switch (sel) {
            case 0: DSA_SPMM_BLOCK(false, false); break;
            case 1: DSA_SPMM_BLOCK(false, true); break;
            case 2: DSA_SPMM_BLOCK(true, false); break;
            default: DSA_SPMM_BLOCK(true, true); break;
        }
#undef DSA_SPMM_BLOCK
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace dsa
