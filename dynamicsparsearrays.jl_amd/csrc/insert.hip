// csrc/insert.hip — K-insert: cells that are NOT STORED yet are created in place from (row, column, value) triples in HBM
// (dsa_mat_insert_batch[_dev]): per orientation one streaming merge of the old cells and the new items into the alternate buffer,
// spread over [1, capacity] the way the root rebalance spreads them.  The back end of update.hip's missing = "skip".
//
// Passes per orientation, on its own stream; the number of launches does not depend on n:
//   (sort)          launch_pair_sort of build.hip: the ops in (partition, inner key, input order) with their input index
//   k_ins_last      one wave: the last occupied slot of the array — the predecessor of every appended partition
//   k_ins_tiles     one wave per tile of INS_TILE slots: its occupied slots
//   k_ins_locate    one lane per sorted op: equal neighbours are duplicates; d_find_table + part_span + d_find (find_dev.h) give the
//                   stored cell (an exact hit) or the predecessor slot — the partition's semaphore when no smaller key exists; a
//                   partition the table does not hold must lie behind its last entry, which must be live.  kind[] = the items the op
//                   adds (0, 1, or 2 with the semaphore of a new partition).  Counts and first errors per workgroup: no atomics.
//   k_ins_verdict   one workgroup: records reduced, workgroup sums and tile counts scanned, INS_PIN_WORDS words to pinned memory
//   k_ins_offsets   per sorted op the items and new partitions in front of it
//   (host: one wait per orientation; an error or a call without an item ends here with nothing written and every plan intact)
//   k_ins_merge_old one wave per tile: predecessor slots do not decrease in sorted order, so the ops behind the slots of a tile are
//                   one contiguous run (two 64-ary searches); their item counts per slot are summed in LDS, an in-tile prefix of
//                   occupancy + items gives every old cell its rank in the merged sequence; cell -> slot spread(rank)
//   k_ins_place_new one lane per sorted op: rank = old cells up to its predecessor + items in front of it; the semaphore of a new
//                   partition (id = table_len + 1 + new partitions in front) one rank in front of its first cell
//   k_ins_bitmap    one lane per destination word: every rank 1 .. m is written by one of the two kernels above, so the occupancy of
//                   the destination is the spread's own (spread_word_bits of dsa_dev.h) — whole words by their only writer, the
//                   same bits on every call, no atomics and no memset
// Keys and values are plain stores by the only writer of a slot.  No float atomics, no atomics on HBM at all.
#include "insert.h"
#include "export_dev.h"

#include <climits>

namespace dsa {

constexpr int INS_WAVES = INS_BLOCK / 64;

__device__ __forceinline__ int64_t ins_wave_min(int64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int64_t y = __shfl_xor(v, o, 64); v = y < v ? y : v; }
    return v;
}
__device__ __forceinline__ uint64_t ins_pack(uint8_t kind) { return (uint64_t)kind | (kind == INS_HEAD ? (1ull << 32) : 0ull); }

__global__ __launch_bounds__(64) void k_ins_last(const uint64_t* __restrict__ occ, int64_t capacity, int64_t* __restrict__ hdr) {
    const int lane = threadIdx.x;
    const int64_t nwords = (capacity + 63) >> 6;
    int64_t last = 0;
    for (int64_t w1 = nwords; w1 > 0; w1 -= 64) {                // words (w1 - 64, w1], lane 0 the highest
        const int64_t w = w1 - 1 - lane;
        const uint64_t word = w >= 0 ? occ[w] : 0ull;
        const uint64_t m = __ballot(word != 0ull);
        if (m) {
            const int l = __ffsll((unsigned long long)m) - 1;
            const uint64_t x = readlane64(word, l);
            last = ((w1 - 1 - l) << 6) + (63 - __clzll((long long)x)) + 1;
            break;
        }
    }
    if (lane == 0) hdr[0] = last <= capacity ? last : capacity;
}

__global__ __launch_bounds__(INS_BLOCK) void k_ins_tiles(const uint64_t* __restrict__ occ, int64_t capacity, uint32_t* __restrict__ tcnt,
                                                        int64_t tiles) {
    const int lane = threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * INS_WAVES + (threadIdx.x >> 6);
    if (t >= tiles) return;
    const int64_t nwords = (capacity + 63) >> 6, w = t * INS_TILE_WORDS + lane;
    uint32_t c = lane < INS_TILE_WORDS && w < nwords ? (uint32_t)popc64(occ[w]) : 0u;
    c = wave_reduce_add(c);
    if (lane == 0) tcnt[t] = c;
}

__global__ __launch_bounds__(INS_BLOCK) void k_ins_locate(SlotView V, int64_t n, InsScratch s, uint8_t* __restrict__ existing) {
    __shared__ int64_t sRec[INS_WAVES][INS_REC_WORDS];
    __shared__ unsigned long long sSum[INS_WAVES];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t j = (int64_t)blockIdx.x * INS_BLOCK + threadIdx.x;
    uint8_t kind = INS_SKIP;
    int64_t n_stored = 0, f_dup = INT64_MAX, f_stored = INT64_MAX, f_mid = INT64_MAX, f_broken = INT64_MAX;
    if (j < n) {
        const int64_t key = s.key[j], part = s.part[j], k = (int64_t)s.idx[j];
        int64_t pred = 0;
        bool stored = false;
        if (j > 0 && s.part[j - 1] == part && s.key[j - 1] == key) {
            f_dup = k;                                                   // the sort is stable: k is the later of the two ops
        } else {
            const DFoundKey f = d_find_table(V.part_keys, V.part_live, V.table_len, part);
            if (f.has && f.key == part) {
                const PartSpan sp = part_span(V, f.pos);
                if (sp.err || sp.from < 1 || sp.to > V.capacity || sp.to < sp.from) {
                    f_broken = k;
                } else {
                    // from = the semaphore's slot (key 0 < key): the answer is a cell of the partition or its semaphore
                    const DFound c = d_find(V.keys, V.vals, V.occ, key, sp.from, sp.to);
                    if (!c.has || c.pos < sp.from || c.pos > sp.to) f_broken = k;
                    else if (c.key == key && c.pos > sp.from) { stored = true; pred = c.pos; n_stored = 1; f_stored = k; }
                    else { pred = c.pos; kind = INS_CELL; }
                }
            } else if (V.table_len == 0 || (V.part_live[V.table_len - 1] != 0 && V.part_keys[V.table_len - 1] < part)) {
                pred = s.hdr[0];
                kind = (j == 0 || s.part[j - 1] != part) ? INS_HEAD : INS_CELL;
            } else {
                f_mid = k;
            }
        }
        s.pred[j] = pred;
        s.kind[j] = kind;
        if (existing != nullptr) existing[k] = stored ? 1 : 0;
    }
    int64_t sum = (int64_t)ins_pack(kind);
    sum = wave_reduce_add(sum); n_stored = wave_reduce_add(n_stored);
    f_dup = ins_wave_min(f_dup); f_stored = ins_wave_min(f_stored); f_mid = ins_wave_min(f_mid); f_broken = ins_wave_min(f_broken);
    if (lane == 0) {
        sSum[wv] = (unsigned long long)sum;
        sRec[wv][0] = n_stored; sRec[wv][1] = 0; sRec[wv][2] = f_dup; sRec[wv][3] = f_stored; sRec[wv][4] = f_mid; sRec[wv][5] = f_broken;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    unsigned long long tot = 0;
    int64_t r[INS_REC_WORDS] = {0, 0, INT64_MAX, INT64_MAX, INT64_MAX, INT64_MAX};
    for (int u = 0; u < INS_WAVES; ++u) {
        tot += sSum[u];
        r[0] += sRec[u][0];
#pragma unroll
        for (int q = 2; q < INS_REC_WORDS; ++q) r[q] = sRec[u][q] < r[q] ? sRec[u][q] : r[q];
    }
    s.bsum[blockIdx.x] = tot;
    int64_t* out = s.rec + (int64_t)blockIdx.x * INS_REC_WORDS;
#pragma unroll
    for (int q = 0; q < INS_REC_WORDS; ++q) out[q] = r[q];
}

// one workgroup, behind k_ins_locate and k_ins_tiles on the stream
__global__ __launch_bounds__(EX_SCAN_THREADS) void k_ins_verdict(InsScratch s, unsigned long long* pinned, unsigned long long seq) {
    __shared__ int64_t sR[EX_SCAN_THREADS / 64][INS_REC_WORDS];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    int64_t v[INS_REC_WORDS] = {0, 0, INT64_MAX, INT64_MAX, INT64_MAX, INT64_MAX};
    for (int64_t b = t; b < s.nblocks; b += EX_SCAN_THREADS) {
#pragma unroll
        for (int q = 0; q < INS_REC_WORDS; ++q) {
            const int64_t x = s.rec[b * INS_REC_WORDS + q];
            v[q] = q < 2 ? v[q] + x : (x < v[q] ? x : v[q]);
        }
    }
#pragma unroll
    for (int q = 0; q < INS_REC_WORDS; ++q) v[q] = q < 2 ? wave_reduce_add(v[q]) : ins_wave_min(v[q]);
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < INS_REC_WORDS; ++q) sR[wv][q] = v[q];
    }
    __syncthreads();
    unsigned long long tot = 0, tot2 = 0, cells = 0, cells2 = 0;
    uint64_t* bsum = s.bsum;
    block_excl_scan2(bsum, bsum, s.nblocks, [bsum](int64_t i, unsigned long long pa, unsigned long long) { bsum[i] = pa; }, tot, tot2);
    int64_t* toff = s.toff;
    block_excl_scan2(s.tcnt, s.tcnt, s.tiles, [toff](int64_t i, unsigned long long pa, unsigned long long) { toff[i] = (int64_t)pa; }, cells, cells2);
    if (t != 0) return;
    for (int u = 1; u < EX_SCAN_THREADS / 64; ++u) {
#pragma unroll
        for (int q = 0; q < INS_REC_WORDS; ++q) v[q] = q < 2 ? v[q] + sR[u][q] : (sR[u][q] < v[q] ? sR[u][q] : v[q]);
    }
    unsigned err = 0;
    if (v[2] != INT64_MAX) err |= INS_E_DUP;
    if (v[3] != INT64_MAX) err |= INS_E_EXISTS;
    if (v[4] != INT64_MAX) err |= INS_E_MIDDLE;
    if (v[5] != INT64_MAX) err |= INS_E_BROKEN;
    s.hdr[1] = (int64_t)cells;
    const unsigned long long w[INS_PIN_WORDS - 1] = {err, (unsigned long long)v[2], (unsigned long long)v[3], (unsigned long long)v[4], (unsigned long long)v[5],
                                                     (unsigned long long)v[0], tot & 0xffffffffull, tot >> 32, cells};
#pragma unroll
    for (int q = 0; q < INS_PIN_WORDS - 1; ++q) __hip_atomic_store(pinned + q, w[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    publish_seq(pinned + INS_PIN_WORDS - 1, seq);
}

// off[j] = (items, new partitions) in front of sorted op j; off[n] = the totals
__global__ __launch_bounds__(INS_BLOCK) void k_ins_offsets(int64_t n, InsScratch s) {
    __shared__ uint32_t sA[INS_WAVES], sB[INS_WAVES];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t j = (int64_t)blockIdx.x * INS_BLOCK + threadIdx.x;
    const uint8_t kind = j < n ? s.kind[j] : INS_SKIP;
    const uint32_t a = kind, b = kind == INS_HEAD ? 1u : 0u;
    const uint32_t ea = wave_excl_scan(a), eb = wave_excl_scan(b);
    if (lane == 63) { sA[wv] = ea + a; sB[wv] = eb + b; }
    __syncthreads();
    uint32_t ba = 0, bb = 0;
    for (int u = 0; u < wv; ++u) { ba += sA[u]; bb += sB[u]; }
    const uint64_t base = s.bsum[blockIdx.x];
    const uint64_t mine = base + (uint64_t)(ba + ea) + ((uint64_t)(bb + eb) << 32);
    if (j < n) s.off[j] = mine;
    if (j == n - 1) s.off[n] = mine + ins_pack(kind);
}

// ---- the merge ------------------------------------------------------------------------------------------------------------------
// 1-based offset of the cell of rank r (1 .. m) after spread! of m cells over g.W slots: the smallest q with q - gaps_le(q) = r.
// cells(q) = q - gaps_le(q) grows by 0 or 1 per offset: a step of r - cells(q) to the right never passes the cell, a step of
// cells(q) - r to the left never falls short of it.
__device__ __forceinline__ int ins_spread_slot(const SpreadGeom& g, int r, double gaps_per_cell) {
    if (g.E <= 0) return r;
    int q = r + (int)((double)(r - 1) * gaps_per_cell);
    if (q < r) q = r;
    if (q > (int)g.W) q = (int)g.W;
#pragma clang loop vectorize(disable) unroll(disable)
    while (true) {
        const int k = gaps_le(g, q);
        const int c = q - k;
        if (c < r) q += r - c;
        else if (c > r) q -= c - r;
        else if (k > 0 && gap_D(g, k) == q) --q;
        else return q;
    }
}

struct InsDst { KeyArr keys; double* vals; int64_t cap; int64_t* sems; int64_t ntab; SpreadGeom g; double gaps_per_cell; };

__device__ __forceinline__ void ins_store(const InsDst& d, int64_t rank, int64_t key, double val) {
    const int64_t q = ins_spread_slot(d.g, (int)rank, d.gaps_per_cell);          // 1-based
    if (q < 1 || q > d.cap) return;
    d.keys[q - 1] = key;
    d.vals[q - 1] = val;
    if (key == SEM_KEY) {
        const int64_t id = (int64_t)val;
        if (id >= 1 && id <= d.ntab) d.sems[id - 1] = q;
    }
}

// the occupancy words of the destination: offsets 64 t + 1 .. 64 t + 64 of the spread, nothing beyond the capacity
__global__ __launch_bounds__(INS_BLOCK) void k_ins_bitmap(uint64_t* __restrict__ occ, int64_t words, SpreadGeom g) {
    const int64_t t = (int64_t)blockIdx.x * INS_BLOCK + threadIdx.x;
    if (t >= words) return;
    uint64_t bits = spread_word_bits(g, (int)t);
    const int64_t left = g.W - 64 * t;
    if (left < 64) bits &= mask_lt((int)left);
    occ[t] = bits;
}

__global__ __launch_bounds__(INS_BLOCK) void k_ins_merge_old(SlotView V, int64_t n, InsScratch s, InsDst d) {
    __shared__ int sAdd[INS_WAVES][INS_TILE];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t t = (int64_t)blockIdx.x * INS_WAVES + wv;
    if (t >= s.tiles) return;                                            // (whole waves: no workgroup barrier below)
    const int64_t nwords = (V.capacity + 63) >> 6, w0 = t * INS_TILE_WORDS;
    uint64_t ow[INS_TILE_WORDS];
    uint64_t any = 0;
#pragma unroll
    for (int jw = 0; jw < INS_TILE_WORDS; ++jw) { ow[jw] = w0 + jw < nwords ? V.occ[w0 + jw] : 0ull; any |= ow[jw]; }
    if (any == 0ull) return;
    const int64_t lo = t * INS_TILE + 1;                                 // the tile's slots: [lo, lo + INS_TILE)
    // (items behind the last occupied slot of the array — every appended partition — move no old cell: they are left out of the sums,
    //  and a batch of new columns costs this wave nothing)
    const int64_t last = s.hdr[0];
    const int64_t hi = last - 1 < lo + INS_TILE - 1 ? (last - 1 > lo - 1 ? last - 1 : lo - 1) : lo + INS_TILE - 1;
    const int64_t i0 = item_past(s.pred, n, lo - 1, lane), i1 = item_past(s.pred, n, hi, lane);
    const bool adds = i1 > i0;
    if (adds) {
        for (int x = lane; x < INS_TILE; x += 64) sAdd[wv][x] = 0;
        for (int64_t j = i0 + lane; j < i1; j += 64) {
            const int c = s.kind[j];
            const int64_t x = s.pred[j] - lo;
            if (c != 0 && x >= 0 && x < INS_TILE) atomicAdd(&sAdd[wv][x], c);      // LDS, integers: any order gives the same sums
        }
        __builtin_amdgcn_wave_barrier();
    }
    int64_t run = s.toff[t] + (int64_t)(s.off[i0] & 0xffffffffull);     // old cells and new items in front of the tile
#pragma unroll
    for (int jw = 0; jw < INS_TILE_WORDS; ++jw) {
        const bool here = (ow[jw] >> lane) & 1ull;
        const uint32_t a = adds ? (uint32_t)sAdd[wv][jw * 64 + lane] : 0u;
        uint32_t before, total;
        if (adds) {
            const uint32_t mine = (here ? 1u : 0u) + a;
            before = wave_excl_scan(mine);
            total = (uint32_t)__shfl((int)(before + mine), 63, 64);
        } else {
            before = (uint32_t)popc64(ow[jw] & mask_lt(lane));
            total = (uint32_t)popc64(ow[jw]);
        }
        if (here) {
            const int64_t slot0 = ((w0 + jw) << 6) + lane;
            ins_store(d, run + before + 1, V.keys.ld(slot0), V.vals[slot0]);
        }
        run += total;
    }
}

__global__ __launch_bounds__(INS_BLOCK) void k_ins_place_new(SlotView V, const double* __restrict__ val, int64_t n, InsScratch s, InsDst d,
                                                            int64_t* __restrict__ part_keys, uint8_t* __restrict__ part_live) {
    const int64_t j = (int64_t)blockIdx.x * INS_BLOCK + threadIdx.x;
    if (j >= n) return;
    const uint8_t kind = s.kind[j];
    if (kind == INS_SKIP) return;
    const int64_t p = s.pred[j];
    int64_t old = 0;                                                     // old cells at slots <= p
    if (p > 0) {
        const int64_t t = (p - 1) / INS_TILE, wp = (p - 1) >> 6;
        old = s.toff[t];
        for (int64_t w = t * INS_TILE_WORDS; w < wp; ++w) old += popc64(V.occ[w]);
        old += popc64(V.occ[wp] & mask_lt((int)((p - 1) & 63) + 1));
    }
    const uint64_t off = s.off[j];
    int64_t rank = old + (int64_t)(off & 0xffffffffull) + 1;
    if (kind == INS_HEAD) {
        const int64_t id = V.table_len + 1 + (int64_t)(off >> 32);
        if (id > d.ntab) return;
        part_keys[id - 1] = s.part[j];
        part_live[id - 1] = 1;
        ins_store(d, rank, SEM_KEY, (double)id);
        ++rank;
    }
    ins_store(d, rank, s.key[j], val[s.idx[j]]);
}

// ---- launch wrappers -----------------------------------------------------------------------------------------------------------
hipError_t launch_insert_prepare(const SlotView& V, const int64_t* d_part, const int64_t* d_key, int64_t n, int64_t pmin, int pbits,
                                 int64_t kmin, int kbits, void* scratch, uint8_t* d_existing, unsigned long long* pinned,
                                 unsigned long long seq, hipStream_t stream) {
    if (n < 1 || n > INT32_MAX || V.capacity < 1 || V.capacity > INT32_MAX || !scratch || !pinned || !V.sems || !V.part_keys || !V.part_live)
        return hipErrorInvalidValue;
    const InsScratch s = ins_carve(scratch, n, V.capacity);
    hipError_t e = launch_pair_sort(d_part, d_key, n, pmin, pbits, kmin, kbits, s.sort, s.idx, s.key, s.part, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_ins_last, dim3(1), dim3(64), 0, stream, V.occ, V.capacity, s.hdr);
    hipLaunchKernelGGL(k_ins_tiles, dim3((unsigned)((s.tiles + INS_WAVES - 1) / INS_WAVES)), dim3(INS_BLOCK), 0, stream, V.occ, V.capacity, s.tcnt,
                       s.tiles);
    hipLaunchKernelGGL(k_ins_locate, dim3((unsigned)s.nblocks), dim3(INS_BLOCK), 0, stream, V, n, s, d_existing);
    hipLaunchKernelGGL(k_ins_verdict, dim3(1), dim3(EX_SCAN_THREADS), 0, stream, s, pinned, seq);
    hipLaunchKernelGGL(k_ins_offsets, dim3((unsigned)s.nblocks), dim3(INS_BLOCK), 0, stream, n, s);
    return hipGetLastError();
}

hipError_t launch_insert_merge(const SlotView& V, const double* d_val, int64_t n, void* scratch, KeyArr dst_keys, double* dst_vals,
                               uint64_t* dst_occ, int64_t dst_cap, int64_t m, int64_t* sems, int64_t* part_keys, uint8_t* part_live,
                               int64_t table_entries, hipStream_t stream) {
    if (n < 1 || n > INT32_MAX || V.capacity < 1 || dst_cap < V.capacity || dst_cap > INT32_MAX || m < 1 || m > dst_cap || !scratch || !sems ||
        !part_keys || !part_live || !d_val || table_entries < V.table_len)
        return hipErrorInvalidValue;
    const InsScratch s = ins_carve(scratch, n, V.capacity);
    InsDst d{dst_keys, dst_vals, dst_cap, sems, table_entries, make_geom(dst_cap, m), (double)(dst_cap - m) / (double)m};
    const int64_t words = (dst_cap + 63) / 64;
    hipLaunchKernelGGL(k_ins_bitmap, dim3((unsigned)((words + INS_BLOCK - 1) / INS_BLOCK)), dim3(INS_BLOCK), 0, stream, dst_occ, words, d.g);
    hipLaunchKernelGGL(k_ins_merge_old, dim3((unsigned)((s.tiles + INS_WAVES - 1) / INS_WAVES)), dim3(INS_BLOCK), 0, stream, V, n, s, d);
    hipLaunchKernelGGL(k_ins_place_new, dim3((unsigned)s.nblocks), dim3(INS_BLOCK), 0, stream, V, d_val, n, s, d, part_keys, part_live);
    return hipGetLastError();
}

}  // namespace dsa
