// csrc/update.hip — K-update: the values of cells that are ALREADY STORED are overwritten (or added to) in place from (row, column,
// value) triples in HBM (dsa_mat_update_values[_dev]), and the batched read that stays in HBM (dsa_mat_get_batch_dev).  No slot
// moves: keys, occupancy words, tables and counters are never written, so the write planner (matwrite_host.hip) is not involved.
// A cell is stored iff the lookup of dsa_mat_get_batch finds it (read.hip: get_one, mode 2): live partition, key equal.
//
// Passes; the number of launches does not depend on n:
//   k_upd_locate   per orientation, on its own stream; one lane per op (256 ops per workgroup): the serial bisections of find_dev.h
//                  (d_find_table, part_span, d_find) give the 1-based slot of the op's cell, or UPD_MISS / UPD_ZERO_KEY / UPD_BROKEN,
//                  into slots[k].  A key 0 is never looked up: it would match a semaphore slot.
//                  Colmajor only, in the same kernel (CLAIM): a located op claims its slot in an open-addressing table of 64-bit
//                  words (update.h: size, hash) — word = slot << 32 | k, atomicCAS on an empty bucket, atomicMax on a bucket that
//                  holds the same slot: the bucket ends with the LARGEST k that addresses the slot, which is what the ops applied
//                  one after the other leave.  Only colmajor slots are claimed: both orientations take their winners from it.
//   k_upd_resolve  colmajor stream, behind both locates (an event): per op the two slots must agree about "stored"; a located op
//                  wins iff its bucket holds its own k -> win[k], d_missing[k].  Misses, winners and the first op of every kind of
//                  error are kept per lane, reduced per wave and stored as the wave's own record: no atomics on a common address.
//   k_upd_verdict  one workgroup: the records reduced (integer sums and minima), eight words to pinned memory
//   (host: one wait; an error or a call without a winner ends here with nothing written and every cached plan intact)
//   k_upd_apply    per orientation: winner k stores V[k] (ADD: vals + V[k], one IEEE add) at vals[slots[k] - 1], a plain 8-byte store by
//                  the slot's only writer; it re-reads the slot's key and never writes a slot that holds the semaphore's key.
// Both orientations store the same V[k] for the same winner: identical bits in every cell, the same bits on every call.
// Bytes per op: locate 16 read (the two keys) + the probes (log2(table_len) table entries, log2(partition slots) bitmap words and keys,
// dependent loads) + 8 written, per orientation; the claim one 8-byte atomic or two; resolve 16 + one bucket read, 1 (+ 1) written;
// apply 1 + 8 read per op and 8 + key (+ 8 for ADD) read, 8 written per winner, per orientation.  Scratch: 17 n + 8 * table bytes.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; no scratch memory in any kernel): see DESIGN.md §3.7.
#include "update.h"
#include "export_dev.h"

#include <climits>

namespace dsa {

constexpr int UPD_VERDICT_THREADS = 1024;
constexpr unsigned long long UPD_K_MASK = (1ull << UPD_K_BITS) - 1ull;

// one lookup by one lane: the probes of get_one (read.hip), the position instead of the value
__device__ int64_t upd_locate_one(const SlotView& V, int64_t key, int64_t part) {
    if (key == SEM_KEY || part == 0) return UPD_ZERO_KEY;
    const DFoundKey f = d_find_table(V.part_keys, V.part_live, V.table_len, part);
    if (!(f.has && f.key == part)) return UPD_MISS;
    const PartSpan sp = part_span(V, f.pos);
    if (sp.err || sp.from < 1 || sp.to > V.capacity) return UPD_BROKEN;
    const DFound c = d_find(V.keys, V.vals, V.occ, key, sp.from, sp.to);
    // behind the semaphore and inside the partition: a negative key bisects to the left of the semaphore, into the partition in front
    return (c.has && c.key == key && c.pos > sp.from && c.pos <= sp.to) ? c.pos : UPD_MISS;
}

__device__ __forceinline__ void upd_claim(const UpdScratch& s, int64_t slot, int64_t k) {
    const unsigned long long word = ((unsigned long long)slot << UPD_K_BITS) | (unsigned long long)k;
    uint64_t p = fib_bucket((uint64_t)slot, s.tshift);
    for (uint64_t i = 0; i <= s.tmask; ++i) {                    // load <= 1/2: an empty bucket always turns up
        unsigned long long cur = __hip_atomic_load(s.table + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == 0ull) {
            cur = atomicCAS(s.table + p, 0ull, word);
            if (cur == 0ull) return;
        }
        if ((cur >> UPD_K_BITS) == (unsigned long long)slot) { atomicMax(s.table + p, word); return; }
        p = (p + 1) & s.tmask;
    }
}
// the k that holds the claim of `slot` (claimed by at least one op of this call), -1 if the table does not know the slot
__device__ __forceinline__ int64_t upd_claimed_by(const UpdScratch& s, int64_t slot) {
    uint64_t p = fib_bucket((uint64_t)slot, s.tshift);
    for (uint64_t i = 0; i <= s.tmask; ++i) {
        const unsigned long long cur = s.table[p];
        if ((cur >> UPD_K_BITS) == (unsigned long long)slot) return (int64_t)(cur & UPD_K_MASK);
        if (cur == 0ull) return -1;
        p = (p + 1) & s.tmask;
    }
    return -1;
}

template <bool CLAIM>
__global__ __launch_bounds__(UPD_BLOCK) void k_upd_locate(SlotView V, const int64_t* __restrict__ key, const int64_t* __restrict__ part,
                                                         int64_t n, UpdScratch s) {
    const int64_t k = (int64_t)blockIdx.x * UPD_BLOCK + threadIdx.x;
    if (k >= n) return;
    const int64_t slot = upd_locate_one(V, key[k], part[k]);
    s.slots[k] = slot;
    if (CLAIM && slot > 0) upd_claim(s, slot, k);
}

__device__ __forceinline__ int64_t wave_min_i64(int64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int64_t y = __shfl_xor(v, o, 64); v = y < v ? y : v; }
    return v;
}

__global__ __launch_bounds__(UPD_BLOCK) void k_upd_resolve(const int64_t* __restrict__ sc, const int64_t* __restrict__ sr, int64_t n,
                                                          UpdScratch s, uint8_t* __restrict__ missing) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * (UPD_BLOCK / 64) + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * (UPD_BLOCK / 64);
    int64_t nmiss = 0, nwin = 0, f_zero = INT64_MAX, f_broken = INT64_MAX, f_miss = INT64_MAX, f_dup = INT64_MAX;
    for (int64_t k = w * 64 + lane; k < n; k += nwaves * 64) {   // k ascends: the first op of a kind is the lane's first
        const int64_t a = sc[k], b = sr[k];
        bool won = false;
        if (a == UPD_ZERO_KEY || b == UPD_ZERO_KEY) { if (f_zero == INT64_MAX) f_zero = k; }
        else if (a == UPD_BROKEN || b == UPD_BROKEN || (a > 0) != (b > 0)) { if (f_broken == INT64_MAX) f_broken = k; }
        else if (a == UPD_MISS) { ++nmiss; if (f_miss == INT64_MAX) f_miss = k; }
        else {
            won = upd_claimed_by(s, a) == k;
            if (won) ++nwin;
            else if (f_dup == INT64_MAX) f_dup = k;
        }
        s.win[k] = won ? 1 : 0;
        if (missing != nullptr) missing[k] = a > 0 ? 0 : 1;
    }
    nmiss = wave_reduce_add(nmiss); nwin = wave_reduce_add(nwin);
    f_zero = wave_min_i64(f_zero); f_broken = wave_min_i64(f_broken); f_miss = wave_min_i64(f_miss); f_dup = wave_min_i64(f_dup);
    if (lane != 0) return;
    int64_t* r = s.rec + w * UPD_REC_WORDS;                      // every wave stores its record: nothing to clear in front
    r[0] = nmiss; r[1] = nwin; r[2] = f_zero; r[3] = f_broken; r[4] = f_miss; r[5] = f_dup;
}

// one workgroup, behind k_upd_resolve on the stream
__global__ __launch_bounds__(UPD_VERDICT_THREADS) void k_upd_verdict(const int64_t* __restrict__ rec, int64_t nrec, int strict, int add,
                                                                    unsigned long long* pinned, unsigned long long seq) {
    __shared__ int64_t sR[UPD_VERDICT_THREADS / 64][UPD_REC_WORDS];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    int64_t v[UPD_REC_WORDS] = {0, 0, INT64_MAX, INT64_MAX, INT64_MAX, INT64_MAX};
    for (int64_t r = t; r < nrec; r += UPD_VERDICT_THREADS) {
#pragma unroll
        for (int q = 0; q < UPD_REC_WORDS; ++q) {
            const int64_t x = rec[r * UPD_REC_WORDS + q];
            v[q] = q < 2 ? v[q] + x : (x < v[q] ? x : v[q]);
        }
    }
#pragma unroll
    for (int q = 0; q < UPD_REC_WORDS; ++q) v[q] = q < 2 ? wave_reduce_add(v[q]) : wave_min_i64(v[q]);
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < UPD_REC_WORDS; ++q) sR[wv][q] = v[q];
    }
    __syncthreads();
    if (t != 0) return;
    for (int u = 1; u < UPD_VERDICT_THREADS / 64; ++u) {
#pragma unroll
        for (int q = 0; q < UPD_REC_WORDS; ++q) v[q] = q < 2 ? v[q] + sR[u][q] : (sR[u][q] < v[q] ? sR[u][q] : v[q]);
    }
    unsigned err = 0;
    if (v[2] != INT64_MAX) err |= UPD_E_ZERO;
    if (v[3] != INT64_MAX) err |= UPD_E_BROKEN;
    if (strict && v[4] != INT64_MAX) err |= UPD_E_MISS;
    if (add && v[5] != INT64_MAX) err |= UPD_E_DUP;
    __hip_atomic_store(pinned + 0, (unsigned long long)err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(pinned + 1, (unsigned long long)v[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(pinned + 2, (unsigned long long)v[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(pinned + 3, (unsigned long long)v[4], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(pinned + 4, (unsigned long long)v[5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(pinned + 5, (unsigned long long)v[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(pinned + 6, (unsigned long long)v[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    publish_seq(pinned + 7, seq);
}

template <bool ADD>
__global__ __launch_bounds__(UPD_BLOCK) void k_upd_apply(KeyArr keys, double* __restrict__ vals, int64_t capacity,
                                                        const double* __restrict__ V, int64_t n, const int64_t* __restrict__ slots,
                                                        const uint8_t* __restrict__ win) {
    const int64_t k = (int64_t)blockIdx.x * UPD_BLOCK + threadIdx.x;
    if (k >= n || win[k] == 0) return;
    const int64_t slot = slots[k];
    if (slot < 1 || slot > capacity) return;
    if (keys.ld(slot - 1) == SEM_KEY) return;                    // a semaphore's value is its partition id: never written from here
    const double v = V[k];
    vals[slot - 1] = ADD ? vals[slot - 1] + v : v;
}

__global__ __launch_bounds__(UPD_BLOCK) void k_upd_get(SlotView V, const int64_t* __restrict__ key, const int64_t* __restrict__ part,
                                                      int64_t n, double* __restrict__ out, uint8_t* __restrict__ found) {
    const int64_t k = (int64_t)blockIdx.x * UPD_BLOCK + threadIdx.x;
    if (k >= n) return;
    const int64_t slot = upd_locate_one(V, key[k], part[k]);
    out[k] = slot > 0 ? V.vals[slot - 1] : 0.0;
    if (found != nullptr) found[k] = slot > 0 ? 1 : 0;
}

// ---- launch wrappers -----------------------------------------------------------------------------------------------------------
static inline unsigned upd_grid(int64_t n) { return (unsigned)((n + UPD_BLOCK - 1) / UPD_BLOCK); }
static inline bool upd_n_ok(int64_t n) { return n >= 1 && (unsigned long long)n <= UPD_K_MASK; }

hipError_t launch_update_locate(const SlotView& V, const int64_t* d_key, const int64_t* d_part, int64_t n, void* scratch, bool colmajor,
                                hipStream_t stream) {
    if (!upd_n_ok(n) || V.capacity < 0 || (V.capacity >> (64 - UPD_K_BITS)) != 0) return hipErrorInvalidValue;
    const UpdScratch s = upd_carve(scratch, n, colmajor);
    if (colmajor) {
        const hipError_t e = hipMemsetAsync(s.table, 0, (size_t)(s.tmask + 1) * sizeof(unsigned long long), stream);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_upd_locate<true>, dim3(upd_grid(n)), dim3(UPD_BLOCK), 0, stream, V, d_key, d_part, n, s);
    } else {
        hipLaunchKernelGGL(k_upd_locate<false>, dim3(upd_grid(n)), dim3(UPD_BLOCK), 0, stream, V, d_key, d_part, n, s);
    }
    return hipGetLastError();
}

hipError_t launch_update_resolve(int64_t n, void* col_scratch, const void* row_scratch, bool strict, bool add, uint8_t* d_missing,
                                 unsigned long long* pinned, unsigned long long seq, hipStream_t stream) {
    if (!upd_n_ok(n)) return hipErrorInvalidValue;
    const UpdScratch s = upd_carve(col_scratch, n, true);
    const UpdScratch r = upd_carve(const_cast<void*>(row_scratch), n, false);
    const unsigned grid = upd_grid(n) < (unsigned)UPD_RESOLVE_BLOCKS ? upd_grid(n) : (unsigned)UPD_RESOLVE_BLOCKS;
    hipLaunchKernelGGL(k_upd_resolve, dim3(grid), dim3(UPD_BLOCK), 0, stream, s.slots, r.slots, n, s, d_missing);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_upd_verdict, dim3(1), dim3(UPD_VERDICT_THREADS), 0, stream, s.rec, (int64_t)grid * (UPD_BLOCK / 64), strict ? 1 : 0,
                       add ? 1 : 0, pinned, seq);
    return hipGetLastError();
}

hipError_t launch_update_apply(KeyArr keys, double* vals, int64_t capacity, const double* d_V, int64_t n, const int64_t* slots,
                               const uint8_t* win, bool add, hipStream_t stream) {
    if (!upd_n_ok(n) || capacity < 0 || !vals || !slots || !win) return hipErrorInvalidValue;
    if (add) hipLaunchKernelGGL(k_upd_apply<true>, dim3(upd_grid(n)), dim3(UPD_BLOCK), 0, stream, keys, vals, capacity, d_V, n, slots, win);
    else hipLaunchKernelGGL(k_upd_apply<false>, dim3(upd_grid(n)), dim3(UPD_BLOCK), 0, stream, keys, vals, capacity, d_V, n, slots, win);
    return hipGetLastError();
}

hipError_t launch_get_batch_dev(const SlotView& V, const int64_t* d_key, const int64_t* d_part, int64_t n, double* d_out, uint8_t* d_found,
                                hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    if (upd_grid(n) == 0 || n > (int64_t)UINT32_MAX * UPD_BLOCK) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_upd_get, dim3(upd_grid(n)), dim3(UPD_BLOCK), 0, stream, V, d_key, d_part, n, d_out, d_found);
    return hipGetLastError();
}

}  // namespace dsa
