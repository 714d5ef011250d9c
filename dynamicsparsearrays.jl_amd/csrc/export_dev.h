// csrc/export_dev.h — what the export kernel units share (compress.hip: the whole orientation, select.hip: the partitions of
// a key list, submatrix.hip: those partitions restricted to an inner key list): the tile they cut the slot array into, the block
// scan between their count and emit launches, and the ends of a scan and of an emit kernel; the tile count of a whole orientation
// (k_cx_count), which compress.hip shares with combine.hip.  For the two key-list exports also the
// whole work-item pipeline: the span kernel of the outer keys (k_key_spans, around key_span of find_dev.h), the owner of a work item (item_past, item_owner), its part of the
// span and its bitmap words (span_chunk, chunk_word), the grid of the item kernels (ex_grid) and the choice of an emit instantiation (dispatch_wide_it).
// Device code, and the two host helpers of its launches.
#pragma once
#include "wave_dev.h"
#include "find_dev.h"
#include <type_traits>

namespace dsa {

constexpr int EX_TILE_SHIFT = 11;                        // 2048 slots = 32 bitmap words: one wave (8192 waves for 2^24 slots)
constexpr int64_t EX_TILE = int64_t(1) << EX_TILE_SHIFT;
constexpr int EX_WORDS = (int)(EX_TILE >> 6);
constexpr int EX_U = 8;                                  // bitmap words whose keys and values a wave requests at once
constexpr int EX_SCAN_THREADS = 1024;
constexpr int64_t EX_BLOCKS_MAX = 4096;                  // grid cap of the work-item kernels: beyond it a thread or wave strides over several
                                                         // units (one ticket per workgroup at the end of an emit: a million of them on one
                                                         // address cost more than the cells)
static inline unsigned ex_grid(int64_t units, int64_t per_block) {
    const int64_t blocks = (units + per_block - 1) / per_block;
    return (unsigned)(blocks < EX_BLOCKS_MAX ? blocks : EX_BLOCKS_MAX);
}

// f(std::bool_constant<WIDE>, IT()) for the key width of the slot array and the caller's index type: the emit kernels are <WIDE, IT>
template <typename F>
static inline void dispatch_wide_it(bool wide, int32_t index_bits, F f) {
    if (wide) {
        if (index_bits == 32) f(std::true_type(), int32_t());
        else f(std::true_type(), int64_t());
    } else {
        if (index_bits == 32) f(std::false_type(), int32_t());
        else f(std::false_type(), int64_t());
    }
}

// One workgroup of EX_SCAN_THREADS: exclusive prefixes of a[0..n) and b[0..n), 8192 entries per step, the sums of the steps in
// front carried along.  put(i, pa, pb) gets the two prefixes of entry i (it may overwrite a[i] and b[i]); the totals come back in
// tot_a / tot_b, the same in every thread.
template <typename T, typename Put>
__device__ __forceinline__ void block_excl_scan2(const T* a, const T* b, int64_t n, Put put, unsigned long long& tot_a,
                                                 unsigned long long& tot_b) {
    __shared__ unsigned long long sO[EX_SCAN_THREADS], sS[EX_SCAN_THREADS];
    const int t = threadIdx.x;
    constexpr int PER = 8;
    unsigned long long carry_o = 0, carry_s = 0;
    for (int64_t c0 = 0; c0 < n; c0 += (int64_t)EX_SCAN_THREADS * PER) {
        unsigned long long vo[PER], vs[PER], to = 0, ts = 0;
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const int64_t i = c0 + (int64_t)t * PER + q;
            vo[q] = i < n ? (unsigned long long)a[i] : 0ull;
            vs[q] = i < n ? (unsigned long long)b[i] : 0ull;
            to += vo[q]; ts += vs[q];
        }
        sO[t] = to; sS[t] = ts;
        __syncthreads();
        for (int o = 1; o < EX_SCAN_THREADS; o <<= 1) {          // inclusive scan (Hillis-Steele)
            const unsigned long long x = t >= o ? sO[t - o] : 0ull, y = t >= o ? sS[t - o] : 0ull;
            __syncthreads();
            sO[t] += x; sS[t] += y;
            __syncthreads();
        }
        unsigned long long ro = carry_o + sO[t] - to, rs = carry_s + sS[t] - ts;
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const int64_t i = c0 + (int64_t)t * PER + q;
            if (i < n) put(i, ro, rs);
            ro += vo[q]; rs += vs[q];
        }
        carry_o += sO[EX_SCAN_THREADS - 1]; carry_s += sS[EX_SCAN_THREADS - 1];
        __syncthreads();
    }
    tot_a = carry_o; tot_b = carry_s;
}

// ---- the tile pass over a whole orientation (compress.hip: CSC / CSR; combine.hip: shifted triples).  Scratch: the four per-tile
// arrays, then the error word and the ticket of the emit (the memset of a launch covers sem_cnt .. ticket)
struct CxScratch {
    int64_t* occ_off; int64_t* sem_off;                  // exclusive prefixes (the scan kernel of the unit)
    uint32_t* occ_cnt; uint32_t* sem_cnt;                // per tile
    uint32_t* err; uint32_t* ticket;
    int64_t tiles;
};
static inline CxScratch cx_carve(void* base, int64_t tiles) {
    CxScratch s;
    s.occ_off = static_cast<int64_t*>(base);
    s.sem_off = s.occ_off + tiles;
    s.occ_cnt = reinterpret_cast<uint32_t*>(s.sem_off + tiles);
    s.sem_cnt = s.occ_cnt + tiles;
    s.err = s.sem_cnt + tiles;
    s.ticket = s.err + 1;
    s.tiles = tiles;
    return s;
}
static inline int64_t cx_tiles(int64_t capacity) { return capacity > 0 ? (capacity + EX_TILE - 1) >> EX_TILE_SHIFT : 1; }
static inline size_t cx_scratch_bytes(int64_t tiles) { return (size_t)tiles * 24 + 8; }

// blocks [0, tile_blocks): four tiles each; the rest: 256 table entries each.  Live semaphores ascend with the id, so the entries of
// a wave fall into few tiles: one atomic per (wave, tile).  With LAST, last_id[t] (zeroed by the caller) also receives the id of the
// last semaphore of tile t, 0 for a tile without one: a tombstoned id has no semaphore and never gets there.  (A template like
// k_key_spans, so that only the units that launch it hold a copy.)
template <bool LAST>
__global__ __launch_bounds__(256) void k_cx_count(const uint64_t* __restrict__ occ, int64_t capacity, const int64_t* __restrict__ sems,
                                                  const uint8_t* __restrict__ col_live, int64_t table_len, int64_t tile_blocks, CxScratch s,
                                                  unsigned long long* __restrict__ last_id) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if ((int64_t)blockIdx.x < tile_blocks) {
        const int64_t t = (int64_t)blockIdx.x * 4 + wv;
        if (t >= s.tiles) return;
        const int64_t w = t * EX_WORDS + lane, nwords = (capacity + 63) >> 6;
        int c = lane < EX_WORDS && w < nwords ? popc64(__builtin_nontemporal_load(occ + w)) : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
        if (lane == 0) s.occ_cnt[t] = (uint32_t)c;
        return;
    }
    const int64_t i = ((int64_t)blockIdx.x - tile_blocks) * 256 + threadIdx.x;
    int64_t tile = -1;
    uint32_t bad = 0;
    if (i < table_len) {
        const int64_t sp = sems[i];
        const bool live = col_live == nullptr || col_live[i] != 0;
        if ((sp != 0) != live || sp < 0 || sp > capacity) bad = 2;          // tables out of step with each other or with the slots
        else if (sp != 0) tile = (sp - 1) >> EX_TILE_SHIFT;
    }
    uint64_t todo = __ballot(tile >= 0);
    while (todo) {
        const int leader = __ffsll((unsigned long long)todo) - 1;
        const int64_t t0 = (int64_t)readlane64((uint64_t)tile, leader);
        const uint64_t m = __ballot(tile == t0);
        if (lane == leader) {
            atomicAdd(s.sem_cnt + t0, (uint32_t)popc64(m));
            if (LAST) atomicMax(last_id + t0, (unsigned long long)(i - lane + (63 - __clzll((unsigned long long)m)) + 1));      // ids ascend with the lane
        }
        todo &= ~m;
    }
    bad = wave_or(bad);
    if (lane == 0 && bad) atomicOr(s.err, bad);
}

// occupied slots of [from, to) (0-based, from < to): the lanes stride over the words, first and last word masked
__device__ __forceinline__ int64_t sel_span_popc(const uint64_t* __restrict__ occ, int64_t from, int64_t to, int lane) {
    int64_t c = 0;
    const int64_t w1 = (to - 1) >> 6;
    for (int64_t w = (from >> 6) + lane; w <= w1; w += 64) c += popc64(occ[w] & word_range_mask(w, from, to - 1));
    return wave_reduce_add(c);
}

// One wave per outer key (4 per workgroup): span j = [lo[j], hi[j]), chunks[j] = 2048-slot tiles of the slot array it touches (0 for a
// span without cells), with CELLS cells[j] = its occupied slots; the error bits of key_span (find_dev.h) are ORed into *err.
template <bool CELLS>
__global__ __launch_bounds__(256) void k_key_spans(SlotView V, const int64_t* __restrict__ keys, int64_t nkeys, int64_t dim_out, int64_t* lo,
                                                   int64_t* hi, int64_t* chunks, int64_t* cells, uint32_t* err) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t j = (int64_t)blockIdx.x * 4 + wv;
    if (j >= nkeys) return;
    const KeySpan sp = key_span(V, keys[j], dim_out, lane);
    const int64_t cnt = sp.hi > sp.lo ? sel_span_popc(V.occ, sp.lo, sp.hi, lane) : 0;
    if (lane != 0) return;
    lo[j] = sp.lo; hi[j] = sp.hi;
    if (CELLS) cells[j] = cnt;
    chunks[j] = cnt > 0 ? ((sp.hi - 1) >> EX_TILE_SHIFT) - (sp.lo >> EX_TILE_SHIFT) + 1 : 0;
    if (sp.err) atomicOr(err, sp.err);
}

// The first key whose item prefix choff[j] exceeds w (n if there is none).  A 64-ary search, one probe per lane and round: prefixes in
// front of L are <= w, the one at H is > w (or H = n).
__device__ __forceinline__ int64_t item_past(const int64_t* __restrict__ choff, int64_t n, int64_t w, int lane) {
    int64_t L = 0, H = n;
    while (H - L > 64) {
        const int64_t width = H - L;
        const int64_t p = L + (width * (lane + 1)) / 64;         // ascending with the lane, lane 63 probes H
        const bool le = p < n && choff[p] <= w;
        const uint64_t nb = ~__ballot(le);
        const int f = nb ? __ffsll((unsigned long long)nb) - 1 : 63;
        H = L + (width * (f + 1)) / 64;
        if (f > 0) L = L + (width * f) / 64 + 1;
    }
    const bool le = L + lane <= H && L + lane < n && choff[L + lane] <= w;
    const uint64_t nb = ~__ballot(le);
    return L + (nb ? __ffsll((unsigned long long)nb) - 1 : 64);
}
// The key that owns work item w: the one in front of item_past (-1 if there is none; choff[0] = 0).  k_sel_emit subtracts the one
// itself: that is the form for which the compiler gives it the instructions of the search it had inline.
__device__ __forceinline__ int64_t item_owner(const int64_t* __restrict__ choff, int64_t n, int64_t w, int lane) {
    return item_past(choff, n, w, lane) - 1;
}

// the part of span [lo, hi) that lies in tile `tile` of the slot array: slots [cs, ce) (ce <= cs: none, the tile is not the span's);
// w0 = the first bitmap word of the tile
struct SpanChunk { int64_t cs, ce, w0; };
__device__ __forceinline__ SpanChunk span_chunk(int64_t lo, int64_t hi, int64_t tile) {
    const int64_t t0 = tile << EX_TILE_SHIFT;
    return SpanChunk{lo > t0 ? lo : t0, hi < t0 + EX_TILE ? hi : t0 + EX_TILE, tile * EX_WORDS};
}
// this lane's bitmap word of the chunk's tile masked to [cs, ce) (0 for a chunk without slots); nz = the words with a cell (a short
// span leaves most groups of a chunk empty)
__device__ __forceinline__ uint64_t chunk_word(const uint64_t* __restrict__ occ, const SpanChunk& c, int lane, uint32_t& nz) {
    uint64_t myword = 0ull;
    if (c.ce > c.cs && lane < EX_WORDS && ((c.w0 + lane) << 6) < c.ce) myword = occ[c.w0 + lane] & word_range_mask(c.w0 + lane, c.cs, c.ce - 1);
    nz = (uint32_t)__ballot(myword != 0ull);
    return myword;
}

// ---- the key block of a key-list operation (submatrix.hip: the inner list; delbatch.hip: the keys to delete): an open-addressing
// hash table of a list of distinct keys >= 1 in pooled scratch — capacity the power of two >= 2 * ninner (load <= 1/2, linear
// probing, Fibonacci hashing), entry = int64 key + int32 position in the list, empty = key 0 — and three arrays of one entry per
// outer key.  Layout: {error word, ticket, 8 bytes of padding}, the table's key words (one memset clears header and key words;
// nothing else is initialised), its positions, then lo / hi / choff.
constexpr uint64_t SUB_NONE = ~0ull;
struct SubKeys {
    uint32_t* err; uint32_t* ticket;
    int64_t* tkey; int32_t* tpos; uint64_t tmask; int tshift;      // entry p of the table; p = (key * phi) >> tshift
    int64_t* lo; int64_t* hi;                            // span of outer key j: slots [lo, hi), 0-based
    int64_t* choff;                                      // work items of j (k_key_spans), then their exclusive prefix
};
static inline uint64_t sub_table_cap(int64_t ninner) {
    uint64_t c = 2;
    while (c < 2 * (uint64_t)(ninner > 0 ? ninner : 0)) c <<= 1;
    return c;
}
static inline SubKeys sub_carve(void* base, int64_t nouter, int64_t ninner) {
    const uint64_t cap = sub_table_cap(ninner);
    SubKeys s;
    s.err = static_cast<uint32_t*>(base);
    s.ticket = s.err + 1;
    s.tkey = reinterpret_cast<int64_t*>(static_cast<char*>(base) + 16);
    s.tpos = reinterpret_cast<int32_t*>(s.tkey + cap);
    s.tmask = cap - 1;
    s.tshift = 64 - __builtin_ctzll(cap);
    s.lo = reinterpret_cast<int64_t*>(s.tpos + cap);     // cap is even: 8-byte aligned
    s.hi = s.lo + nouter;
    s.choff = s.hi + nouter;
    return s;
}
static inline size_t sub_key_block_bytes(int64_t nouter, int64_t ninner) {
    return 16 + (size_t)sub_table_cap(ninner) * 12 + (size_t)(nouter > 0 ? nouter : 0) * 24;
}
static inline size_t sub_key_block_clear_bytes(const SubKeys& s) { return 16 + (size_t)(s.tmask + 1) * 8; }      // error word, ticket, every key word

// Fibonacci hashing into a table of 2^(64 - shift) entries: the first entry a key probes in every open-addressing table of the
// library (the key tables here, the claim table of update.hip); a probe moves on by one entry, wrapping at the end
__device__ __forceinline__ uint64_t fib_bucket(uint64_t key, int shift) { return (key * 0x9E3779B97F4A7C15ull) >> shift; }
__device__ __forceinline__ uint64_t sub_slot(const SubKeys& s, int64_t key) { return fib_bucket((uint64_t)key, s.tshift); }
// the entry that holds `key` (>= 1), given the key word t already loaded from its first entry p; SUB_NONE if the key is not listed
__device__ __forceinline__ uint64_t sub_resolve(const SubKeys& s, int64_t key, uint64_t p, int64_t t) {
    for (uint64_t n = 0; n <= s.tmask; ++n) {
        if (t == key) return p;
        if (t == 0) return SUB_NONE;
        p = (p + 1) & s.tmask;
        t = s.tkey[p];
    }
    return SUB_NONE;
}

// grid-wide over the list: range check (error bit 4), 64-bit atomicCAS on the key word of the probed entry; a CAS that meets its
// own key again is the repeated-key error (bit 8).  (A template like k_key_spans, so that only the units that launch it hold a copy.)
template <int UNUSED = 0>
__global__ __launch_bounds__(256) void k_sub_hash(const int64_t* __restrict__ inner, int64_t ninner, int64_t dim_in, SubKeys s) {
    uint32_t err = 0;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < ninner; i += stride) {
        const int64_t key = inner[i];
        if (key < 1 || key > dim_in) { err |= 4u; continue; }
        uint64_t p = sub_slot(s, key);
        for (uint64_t n = 0; n <= s.tmask; ++n) {                // load <= 1/2: an empty entry always turns up
            const unsigned long long old = atomicCAS(reinterpret_cast<unsigned long long*>(s.tkey + p), 0ull, (unsigned long long)key);
            if (old == 0ull) { s.tpos[p] = (int32_t)i; break; }
            if (old == (unsigned long long)key) { err |= 8u; break; }
            p = (p + 1) & s.tmask;
        }
    }
    if (err) atomicOr(s.err, err);
}

// The hand-over at the end of a scan or emit kernel (one thread).  The pinned words by n, the number of totals the host expects:
//   n = 0  {error word, seq}     n = 1  {error word, t0, seq}     n = 2  {error word, t0, t1, seq}
// n must be the literal the host side's wait_handover(pin + n + 1) goes with: seq lands behind the totals.
__device__ __forceinline__ void hand_over(const uint32_t* err_word, unsigned long long* pinned, unsigned long long seq, int n = 0,
                                          unsigned long long t0 = 0, unsigned long long t1 = 0) {
    const uint32_t e = __hip_atomic_load(err_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(pinned + 0, (unsigned long long)e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (n > 0) __hip_atomic_store(pinned + 1, t0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (n > 1) __hip_atomic_store(pinned + 2, t1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    publish_seq(pinned + n + 1, seq);
}

// The end of an emit kernel (256 threads, every one arrives): the error bits of the workgroup go into the scratch word, and the
// workgroup that takes the last ticket hands {error word, seq} to pinned memory (emit_epilogue).  emit_last is the part in front of
// the hand-over for an emit with more to hand over than the error word: true in the one thread that has to do it.
__device__ __forceinline__ bool emit_last(uint32_t err, int lane, int wv, uint32_t* err_word, uint32_t* ticket) {
    __shared__ uint32_t sErr[4];
    err = wave_or(err);
    if (lane == 0) sErr[wv] = err;
    __syncthreads();
    if (threadIdx.x != 0) return false;
    err = sErr[0] | sErr[1] | sErr[2] | sErr[3];
    if (err) __hip_atomic_fetch_or(err_word, err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_s_waitcnt(0);
    const uint32_t tk = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return tk == gridDim.x - 1;                                  // the last workgroup: every other one has added its bits before its ticket
}
__device__ __forceinline__ void emit_epilogue(uint32_t err, int lane, int wv, uint32_t* err_word, uint32_t* ticket,
                                              unsigned long long* pinned, unsigned long long seq) {
    if (emit_last(err, lane, wv, err_word, ticket)) hand_over(err_word, pinned, seq);
}

}  // namespace dsa
