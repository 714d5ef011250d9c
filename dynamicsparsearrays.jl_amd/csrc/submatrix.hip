// csrc/submatrix.hip — K-submatrix: A[I, J] with both key lists as one compressed matrix (A[inner, outer] as CSC from colmajor,
// A[outer, inner] as CSR from rowmajor), cost proportional to the selected partitions and the two lists.
//
// The OUTER list picks partitions exactly as the selected export does (select.hip: any order, repeats allowed, a key without a live
// partition gives an empty slice).  The INNER list (distinct keys, any order) decides which cells of those partitions are kept and
// renumbers them: a kept cell's index is the 0-based position of its key in the inner list (+ base).  Within a slice the kept cells
// stay in slot order, i.e. ascending ORIGINAL inner key.
//
// Inner-key lookup, one structure for every case: an open-addressing hash table in pooled scratch, capacity the power of two
// >= 2 * ninner (load <= 1/2, linear probing, Fibonacci hashing), entry = int64 key + int32 position, empty = key 0 (a listed key
// is >= 1).  One memset clears the key words together with the error word; nothing else is initialised.  Nothing is proportional
// to dim_in (which exceeds 2^31 with wide keys) or to the capacity.
//
// Six launches, three host waits, whatever nouter, ninner and the span lengths are:
//   k_sub_hash        grid-wide over the inner list: range check, 64-bit atomicCAS on the key word of the probed entry; a CAS that
//                     meets its own key again is the repeated-key error
//   k_sub_spans       one wave per outer key: the span (export_dev.h: key_span, shared with k_sel_count) and the 2048-slot tiles of
//                     the slot array it touches (0 for a span without cells)
//   k_sub_scan_items  one workgroup: exclusive prefix of the tiles -> the first work item of every outer key; {error word, items}
//                     go to pinned memory
//   (host: waits for the item count, sizes the item block)
//   k_sub_count       one wave per work item (outer j, tile c), j by an upper-bound search over the item prefix: loads the keys of
//                     the occupied slots, probes the table, counts the kept cells by ballot / popcount; stored keys outside
//                     1..dim_in are found here.  Writes kept[w] and owner[w]
//   k_sub_scan_cells  one workgroup: exclusive prefix of kept[] -> the output offset of every work item; ptr[j] = base + the offset
//                     of j's first item; {error word, total} go to pinned memory
//   (host: waits for the total, checks cap and the 32-bit rule)
//   k_sub_emit        one wave per work item with kept cells: keys loaded non-temporally, the probes of EX_U bitmap words issued
//                     before the first is consumed, kept cells compacted by ballot / popcount ranks at item offset + rank, values
//                     loaded for kept cells only, idx / vals stored non-temporally; the last workgroup hands the error word over
// No wave owns a whole long partition.  No atomics on the output and no floating-point arithmetic: a cell's place depends on the
// slot order and on WHETHER a key is in the table, never on where the hash put it, so the result is bit-identical from call to call.
// Bytes in: 8 * (nouter + ninner) keys, 8 * log2(table_len) probed table bytes per outer key, per slot of the selected spans its
// key twice (kb, count and emit) and one 8-byte table probe each time (one 64-byte line at load 1/2 in the common case), 8 + 4
// bytes per KEPT cell (value, position), the spans' bitmap words twice.  Bytes out: 12 * table capacity (<= 48 * ninner),
// (ib + 8) * total + ib * (nouter + 1).
#include "submatrix.h"
#include "export_dev.h"
#include <type_traits>

namespace dsa {

constexpr int64_t SUB_BLOCKS_MAX = 4096;                 // grid cap of the grid-strided kernels (the reason SEL_EMIT_BLOCKS_MAX has)
constexpr uint64_t SUB_NONE = ~0ull;

// key block: {error word, ticket of the emit, 8 bytes of padding}, the table's key words (the memset ends behind them), its
// positions, then three arrays of nouter entries
struct SubKeys {
    uint32_t* err; uint32_t* ticket;
    int64_t* tkey; int32_t* tpos; uint64_t tmask; int tshift;      // entry p of the table; p = (key * phi) >> tshift
    int64_t* lo; int64_t* hi;                            // span of outer key j: slots [lo, hi), 0-based
    int64_t* choff;                                      // work items of j (k_sub_spans), then their exclusive prefix
};
// item block
struct SubItems {
    int64_t* off;                                        // kept cells of item w (k_sub_count), then their exclusive prefix
    int32_t* owner;                                      // the outer index j the item belongs to
};

static uint64_t sub_table_cap(int64_t ninner) {
    uint64_t c = 2;
    while (c < 2 * (uint64_t)(ninner > 0 ? ninner : 0)) c <<= 1;
    return c;
}
static SubKeys sub_carve(void* base, int64_t nouter, int64_t ninner) {
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
static SubItems sub_carve_items(void* base, int64_t items) {
    SubItems it;
    it.off = static_cast<int64_t*>(base);
    it.owner = reinterpret_cast<int32_t*>(it.off + items);
    return it;
}
size_t submatrix_key_scratch_bytes(int64_t nouter, int64_t ninner) {
    return 16 + (size_t)sub_table_cap(ninner) * 12 + (size_t)(nouter > 0 ? nouter : 0) * 24;
}
size_t submatrix_item_scratch_bytes(int64_t items) { return (size_t)(items > 0 ? items : 0) * 12 + 16; }

__device__ __forceinline__ uint64_t sub_slot(const SubKeys& s, int64_t key) {
    return ((uint64_t)key * 0x9E3779B97F4A7C15ull) >> s.tshift;
}
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

// grid-wide over the inner list
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

// one wave per outer key
__global__ __launch_bounds__(256) void k_sub_spans(const uint64_t* __restrict__ occ, int64_t capacity, const int64_t* __restrict__ sems,
                                                   const int64_t* __restrict__ col_keys, const uint8_t* __restrict__ col_live,
                                                   int64_t table_len, bool dense, const int64_t* __restrict__ outer, int64_t nouter,
                                                   int64_t dim_out, SubKeys s) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t j = (int64_t)blockIdx.x * 4 + wv;
    if (j >= nouter) return;
    const KeySpan sp = key_span(capacity, sems, col_keys, col_live, table_len, dense, outer[j], dim_out, lane);
    const int64_t cnt = sp.hi > sp.lo ? sel_span_popc(occ, sp.lo, sp.hi, lane) : 0;
    if (lane != 0) return;
    s.lo[j] = sp.lo; s.hi[j] = sp.hi;
    s.choff[j] = cnt > 0 ? ((sp.hi - 1) >> EX_TILE_SHIFT) - (sp.lo >> EX_TILE_SHIFT) + 1 : 0;
    if (sp.err) atomicOr(s.err, sp.err);
}

// one workgroup: choff becomes its exclusive prefix in place
__global__ __launch_bounds__(EX_SCAN_THREADS) void k_sub_scan_items(SubKeys s, int64_t nouter, unsigned long long* pinned,
                                                                    unsigned long long seq) {
    unsigned long long items, same;
    block_excl_scan2(s.choff, s.choff, nouter, [&](int64_t i, unsigned long long r, unsigned long long) { s.choff[i] = (int64_t)r; },
                     items, same);
    if (threadIdx.x != 0) return;
    const uint32_t e = __hip_atomic_load(s.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(pinned + 0, (unsigned long long)e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(pinned + 1, items, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    publish_seq(pinned + 2, seq);
}

// The outer index that owns work item w: the last j whose item prefix is <= w (-1 if there is none).  A 64-ary search, one probe per
// lane and round: prefixes in front of L are <= w, the one at H is > w (or H = n).  The search k_sel_emit makes over its chunk prefix.
__device__ __forceinline__ int64_t sub_item_owner(const int64_t* __restrict__ choff, int64_t n, int64_t w, int lane) {
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
    return L + (nb ? __ffsll((unsigned long long)nb) - 1 : 64) - 1;
}

// the part of span [lo, hi) that lies in tile `tile` of the slot array: slots [cs, ce), this lane's bitmap word of the tile masked
// to them, and the words with a cell
struct SubChunk { int64_t cs, ce, w0; uint64_t myword; uint32_t nz; };
__device__ __forceinline__ SubChunk sub_chunk(const uint64_t* __restrict__ occ, int64_t lo, int64_t hi, int64_t tile, int lane) {
    SubChunk c;
    const int64_t t0 = tile << EX_TILE_SHIFT;
    c.cs = lo > t0 ? lo : t0;
    c.ce = hi < t0 + EX_TILE ? hi : t0 + EX_TILE;
    c.w0 = tile * EX_WORDS;
    c.myword = 0ull;
    if (c.ce > c.cs && lane < EX_WORDS && ((c.w0 + lane) << 6) < c.ce) c.myword = occ[c.w0 + lane] & word_range_mask(c.w0 + lane, c.cs, c.ce - 1);
    c.nz = (uint32_t)__ballot(c.myword != 0ull);
    return c;
}

// one wave per work item
template <bool WIDE>
__global__ __launch_bounds__(256) void k_sub_count(KeyArr keys, const uint64_t* __restrict__ occ, SubKeys s, SubItems it, int64_t nouter,
                                                   int64_t items, int64_t dim_in) {
    typedef typename std::conditional<WIDE, int64_t, int32_t>::type key_t;
    const key_t* __restrict__ kp = static_cast<const key_t*>(keys.p);
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    uint32_t err = 0;
    for (int64_t w = (int64_t)blockIdx.x * 4 + wv; w < items; w += nwaves) {
        int64_t j = sub_item_owner(s.choff, nouter, w, lane);
        int64_t cnt = 0;
        if (j < 0 || j >= nouter) {
            err |= 2u; j = 0;
        } else {
            const int64_t lo = s.lo[j], hi = s.hi[j];
            const SubChunk c = sub_chunk(occ, lo, hi, (lo >> EX_TILE_SHIFT) + (w - s.choff[j]), lane);
            if (c.ce <= c.cs) err |= 2u;
            for (int q = 0; q < EX_WORDS; q += EX_U) {
                if (((c.nz >> q) & ((1u << EX_U) - 1u)) == 0u) continue;
                int64_t k[EX_U], t[EX_U];
                uint64_t p[EX_U];
                bool ok[EX_U];
#pragma unroll
                for (int u = 0; u < EX_U; ++u) {
                    const bool cell = (readlane64(c.myword, q + u) >> lane) & 1ull;
                    k[u] = 0;
                    if (cell) k[u] = (int64_t)kp[((c.w0 + q + u) << 6) + lane];
                    ok[u] = cell && k[u] >= 1 && k[u] <= dim_in;
                    if (cell && !ok[u]) err |= k[u] == SEM_KEY ? 2u : 16u;      // a semaphore inside a span, or a cell outside size(m)
                }
#pragma unroll
                for (int u = 0; u < EX_U; ++u) {
                    p[u] = 0; t[u] = 0;
                    if (ok[u]) { p[u] = sub_slot(s, k[u]); t[u] = s.tkey[p[u]]; }
                }
#pragma unroll
                for (int u = 0; u < EX_U; ++u) {
                    const bool kept = ok[u] && sub_resolve(s, k[u], p[u], t[u]) != SUB_NONE;
                    cnt += popc64(__ballot(kept));
                }
            }
        }
        if (lane == 0) { it.off[w] = cnt; it.owner[w] = (int32_t)j; }
    }
    err = wave_or(err);
    if (lane == 0 && err) atomicOr(s.err, err);
}

// one workgroup: off becomes its exclusive prefix in place, ptr[j] = base + off[first item of j] (total behind the last item)
template <typename IT>
__global__ __launch_bounds__(EX_SCAN_THREADS) void k_sub_scan_cells(SubKeys s, SubItems it, int64_t nouter, int64_t items, int64_t base,
                                                                    IT* __restrict__ ptr, unsigned long long* pinned,
                                                                    unsigned long long seq) {
    unsigned long long total, same;
    block_excl_scan2(it.off, it.off, items, [&](int64_t i, unsigned long long r, unsigned long long) { it.off[i] = (int64_t)r; },
                     total, same);
    for (int64_t j = threadIdx.x; j < nouter; j += EX_SCAN_THREADS) {
        const int64_t f = s.choff[j];
        ptr[j] = (IT)(base + (f >= 0 && f < items ? it.off[f] : (int64_t)total));
    }
    if (threadIdx.x != 0) return;
    ptr[nouter] = (IT)(base + (int64_t)total);
    const uint32_t e = __hip_atomic_load(s.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(pinned + 0, (unsigned long long)e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(pinned + 1, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    publish_seq(pinned + 2, seq);
}

struct SubArgs {
    void* idx; double* val;
    int64_t nouter, items, total, base;
    unsigned long long* pinned;         // {error word, sequence number}
    unsigned long long seq;
};

// one wave per work item.  Error bit 2: the emit keeps other cells than the count did.
template <bool WIDE, typename IT>
__global__ __launch_bounds__(256) void k_sub_emit(KeyArr keys, const double* __restrict__ vals, const uint64_t* __restrict__ occ, SubKeys s,
                                                  SubItems it, SubArgs a) {
    typedef typename std::conditional<WIDE, int64_t, int32_t>::type key_t;
    const key_t* __restrict__ kp = static_cast<const key_t*>(keys.p);
    IT* __restrict__ idx = static_cast<IT*>(a.idx);
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t below = mask_lt(lane);
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    uint32_t err = 0;
    for (int64_t w = (int64_t)blockIdx.x * 4 + wv; w < a.items; w += nwaves) {
        int64_t run = it.off[w];
        const int64_t end = w + 1 < a.items ? it.off[w + 1] : a.total;
        if (end <= run) continue;                                // nothing of this item is kept: its keys are not read again
        const int64_t j = it.owner[w];
        if (j < 0 || j >= a.nouter || end > a.total) { err |= 2u; continue; }
        const int64_t lo = s.lo[j], hi = s.hi[j];
        const SubChunk c = sub_chunk(occ, lo, hi, (lo >> EX_TILE_SHIFT) + (w - s.choff[j]), lane);
        for (int q = 0; q < EX_WORDS; q += EX_U) {
            if (((c.nz >> q) & ((1u << EX_U) - 1u)) == 0u) continue;
            int64_t k[EX_U], t[EX_U], out[EX_U];
            uint64_t p[EX_U];
            int32_t pos[EX_U];
            double v[EX_U];
#pragma unroll
            for (int u = 0; u < EX_U; ++u) {
                k[u] = 0;
                if ((readlane64(c.myword, q + u) >> lane) & 1ull) k[u] = (int64_t)__builtin_nontemporal_load(kp + ((c.w0 + q + u) << 6) + lane);
            }
#pragma unroll
            for (int u = 0; u < EX_U; ++u) {                     // every first probe is on its way before one is looked at
                p[u] = 0; t[u] = 0;
                if (k[u] >= 1) { p[u] = sub_slot(s, k[u]); t[u] = s.tkey[p[u]]; }
            }
#pragma unroll
            for (int u = 0; u < EX_U; ++u) {
                p[u] = k[u] >= 1 ? sub_resolve(s, k[u], p[u], t[u]) : SUB_NONE;
                const uint64_t m = __ballot(p[u] != SUB_NONE);
                out[u] = run + popc64(m & below);
                run += popc64(m);
                pos[u] = 0; v[u] = 0.0;
                if (p[u] != SUB_NONE) {
                    pos[u] = s.tpos[p[u]];
                    v[u] = __builtin_nontemporal_load(vals + ((c.w0 + q + u) << 6) + lane);
                }
            }
#pragma unroll
            for (int u = 0; u < EX_U; ++u) {
                if (p[u] != SUB_NONE) {
                    if (out[u] >= end) {
                        err |= 2u;
                    } else {
                        __builtin_nontemporal_store((IT)((int64_t)pos[u] + a.base), idx + out[u]);
                        __builtin_nontemporal_store(v[u], a.val + out[u]);
                    }
                }
            }
        }
        if (run != end) err |= 2u;
    }
    emit_epilogue(err, lane, wv, s.err, s.ticket, a.pinned, a.seq);
}

static unsigned sub_grid(int64_t units, int64_t per_block) {
    const int64_t blocks = (units + per_block - 1) / per_block;
    return (unsigned)(blocks < SUB_BLOCKS_MAX ? blocks : SUB_BLOCKS_MAX);
}

hipError_t launch_submatrix_keys(const uint64_t* occ, int64_t capacity, const int64_t* sems, const int64_t* col_keys, const uint8_t* col_live,
                                 int64_t table_len, bool dense, const int64_t* d_outer, int64_t nouter, int64_t dim_out,
                                 const int64_t* d_inner, int64_t ninner, int64_t dim_in, void* key_scratch, unsigned long long* pinned3,
                                 unsigned long long seq, hipStream_t stream) {
    if (capacity < 0 || table_len < 0 || nouter < 0 || nouter > INT32_MAX || ninner < 0 || ninner > INT32_MAX) return hipErrorInvalidValue;
    const SubKeys s = sub_carve(key_scratch, nouter, ninner);
    hipError_t e = hipMemsetAsync(key_scratch, 0, 16 + (size_t)(s.tmask + 1) * 8, stream);      // error word, ticket, every key word
    if (e != hipSuccess) return e;
    if (ninner > 0) hipLaunchKernelGGL(k_sub_hash, dim3(sub_grid(ninner, 256)), dim3(256), 0, stream, d_inner, ninner, dim_in, s);
    if (nouter > 0)
        hipLaunchKernelGGL(k_sub_spans, dim3((unsigned)((nouter + 3) / 4)), dim3(256), 0, stream, occ, capacity, sems, col_keys, col_live,
                           table_len, dense || col_live == nullptr, d_outer, nouter, dim_out, s);
    hipLaunchKernelGGL(k_sub_scan_items, dim3(1), dim3(EX_SCAN_THREADS), 0, stream, s, nouter, pinned3, seq);
    return hipGetLastError();
}

hipError_t launch_submatrix_count(KeyArr keys, const uint64_t* occ, int64_t capacity, int64_t nouter, int64_t ninner, int64_t items,
                                  int64_t dim_in, int32_t index_bits, int64_t base, void* d_ptr, void* key_scratch, void* item_scratch,
                                  unsigned long long* pinned3, unsigned long long seq, hipStream_t stream) {
    if (capacity < 0 || nouter < 0 || ninner < 0 || items < 0 || (index_bits != 32 && index_bits != 64)) return hipErrorInvalidValue;
    const SubKeys s = sub_carve(key_scratch, nouter, ninner);
    const SubItems it = sub_carve_items(item_scratch, items);
    if (items > 0) {
        const unsigned grid = sub_grid(items, 4);
        if (keys.wide) hipLaunchKernelGGL(k_sub_count<true>, dim3(grid), dim3(256), 0, stream, keys, occ, s, it, nouter, items, dim_in);
        else hipLaunchKernelGGL(k_sub_count<false>, dim3(grid), dim3(256), 0, stream, keys, occ, s, it, nouter, items, dim_in);
    }
    if (index_bits == 32)
        hipLaunchKernelGGL(k_sub_scan_cells<int32_t>, dim3(1), dim3(EX_SCAN_THREADS), 0, stream, s, it, nouter, items, base,
                           static_cast<int32_t*>(d_ptr), pinned3, seq);
    else
        hipLaunchKernelGGL(k_sub_scan_cells<int64_t>, dim3(1), dim3(EX_SCAN_THREADS), 0, stream, s, it, nouter, items, base,
                           static_cast<int64_t*>(d_ptr), pinned3, seq);
    return hipGetLastError();
}

template <bool WIDE, typename IT>
static void launch_sub_emit_t(unsigned grid, hipStream_t stream, KeyArr keys, const double* vals, const uint64_t* occ, const SubKeys& s,
                              const SubItems& it, const SubArgs& a) {
    hipLaunchKernelGGL((k_sub_emit<WIDE, IT>), dim3(grid), dim3(256), 0, stream, keys, vals, occ, s, it, a);
}

hipError_t launch_submatrix_emit(KeyArr keys, const double* vals, const uint64_t* occ, int64_t capacity, int64_t nouter, int64_t ninner,
                                 int64_t items, int64_t total, int32_t index_bits, int64_t base, void* d_idx, double* d_vals,
                                 void* key_scratch, void* item_scratch, unsigned long long* pinned2, unsigned long long seq,
                                 hipStream_t stream) {
    if (capacity < 0 || nouter < 1 || ninner < 1 || items < 1 || total < 1 || (index_bits != 32 && index_bits != 64)) return hipErrorInvalidValue;
    const SubKeys s = sub_carve(key_scratch, nouter, ninner);
    const SubItems it = sub_carve_items(item_scratch, items);
    const SubArgs a{d_idx, d_vals, nouter, items, total, base, pinned2, seq};
    const unsigned grid = sub_grid(items, 4);
    if (keys.wide) {
        if (index_bits == 32) launch_sub_emit_t<true, int32_t>(grid, stream, keys, vals, occ, s, it, a);
        else launch_sub_emit_t<true, int64_t>(grid, stream, keys, vals, occ, s, it, a);
    } else {
        if (index_bits == 32) launch_sub_emit_t<false, int32_t>(grid, stream, keys, vals, occ, s, it, a);
        else launch_sub_emit_t<false, int64_t>(grid, stream, keys, vals, occ, s, it, a);
    }
    return hipGetLastError();
}

}  // namespace dsa
