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
//   k_key_spans       one wave per outer key: the span and the 2048-slot tiles of the slot array it touches (0 for a span without
//                     cells); the kernel of the selected export (export_dev.h), without its cell counts
//   k_sub_scan_items  one workgroup: exclusive prefix of the tiles -> the first work item of every outer key; {error word, items}
//                     go to pinned memory
//   (host: waits for the item count, sizes the item block)
//   k_sub_count       one wave per work item (outer j, tile c), j by an upper-bound search over the item prefix (item_owner), its
//                     slots and bitmap words by span_chunk / chunk_word (all in export_dev.h, shared with k_sel_emit): loads the keys of
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

namespace dsa {

// SubKeys, the key block (hash table of the inner list, spans of the outer list), its carving and k_sub_hash are in export_dev.h:
// the batched delete (delbatch.hip) puts its key list into the same table

// item block
struct SubItems {
    int64_t* off;                                        // kept cells of item w (k_sub_count), then their exclusive prefix
    int32_t* owner;                                      // the outer index j the item belongs to
};

static SubItems sub_carve_items(void* base, int64_t items) {
    SubItems it;
    it.off = static_cast<int64_t*>(base);
    it.owner = reinterpret_cast<int32_t*>(it.off + items);
    return it;
}
size_t submatrix_key_scratch_bytes(int64_t nouter, int64_t ninner) { return sub_key_block_bytes(nouter, ninner); }
size_t submatrix_item_scratch_bytes(int64_t items) { return (size_t)(items > 0 ? items : 0) * 12 + 16; }

// one workgroup: choff becomes its exclusive prefix in place
__global__ __launch_bounds__(EX_SCAN_THREADS) void k_sub_scan_items(SubKeys s, int64_t nouter, unsigned long long* pinned,
                                                                    unsigned long long seq) {
    unsigned long long items, same;
    block_excl_scan2(s.choff, s.choff, nouter, [&](int64_t i, unsigned long long r, unsigned long long) { s.choff[i] = (int64_t)r; },
                     items, same);
    if (threadIdx.x != 0) return;
    hand_over(s.err, pinned, seq, 1, items);
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
        int64_t j = item_owner(s.choff, nouter, w, lane);
        int64_t cnt = 0;
        if (j < 0 || j >= nouter) {
            err |= 2u; j = 0;
        } else {
            const int64_t lo = s.lo[j], hi = s.hi[j];
            const SpanChunk c = span_chunk(lo, hi, (lo >> EX_TILE_SHIFT) + (w - s.choff[j]));
            uint32_t nz;
            const uint64_t myword = chunk_word(occ, c, lane, nz);
            if (c.ce <= c.cs) err |= 2u;
            for (int q = 0; q < EX_WORDS; q += EX_U) {
                if (((nz >> q) & ((1u << EX_U) - 1u)) == 0u) continue;
                int64_t k[EX_U], t[EX_U];
                uint64_t p[EX_U];
                bool ok[EX_U];
#pragma unroll
                for (int u = 0; u < EX_U; ++u) {
                    const bool cell = (readlane64(myword, q + u) >> lane) & 1ull;
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
    hand_over(s.err, pinned, seq, 1, total);
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
        const SpanChunk c = span_chunk(lo, hi, (lo >> EX_TILE_SHIFT) + (w - s.choff[j]));
        uint32_t nz;
        const uint64_t myword = chunk_word(occ, c, lane, nz);
        for (int q = 0; q < EX_WORDS; q += EX_U) {
            if (((nz >> q) & ((1u << EX_U) - 1u)) == 0u) continue;
            int64_t k[EX_U], t[EX_U], out[EX_U];
            uint64_t p[EX_U];
            int32_t pos[EX_U];
            double v[EX_U];
#pragma unroll
            for (int u = 0; u < EX_U; ++u) {
                k[u] = 0;
                if ((readlane64(myword, q + u) >> lane) & 1ull) k[u] = (int64_t)__builtin_nontemporal_load(kp + ((c.w0 + q + u) << 6) + lane);
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

hipError_t launch_submatrix_keys(const SlotView& V, const int64_t* d_outer, int64_t nouter, int64_t dim_out, const int64_t* d_inner,
                                 int64_t ninner, int64_t dim_in, void* key_scratch, unsigned long long* pinned3, unsigned long long seq,
                                 hipStream_t stream) {
    if (V.capacity < 0 || V.table_len < 0 || nouter < 0 || nouter > INT32_MAX || ninner < 0 || ninner > INT32_MAX) return hipErrorInvalidValue;
    const SubKeys s = sub_carve(key_scratch, nouter, ninner);
    hipError_t e = hipMemsetAsync(key_scratch, 0, sub_key_block_clear_bytes(s), stream);
    if (e != hipSuccess) return e;
    if (ninner > 0) hipLaunchKernelGGL(k_sub_hash<>, dim3(ex_grid(ninner, 256)), dim3(256), 0, stream, d_inner, ninner, dim_in, s);
    if (nouter > 0)
        hipLaunchKernelGGL(k_key_spans<false>, dim3((unsigned)((nouter + 3) / 4)), dim3(256), 0, stream, V, d_outer, nouter, dim_out, s.lo, s.hi,
                           s.choff, (int64_t*)nullptr, s.err);
    hipLaunchKernelGGL(k_sub_scan_items, dim3(1), dim3(EX_SCAN_THREADS), 0, stream, s, nouter, pinned3, seq);
    return hipGetLastError();
}

hipError_t launch_submatrix_count(const SlotView& V, int64_t nouter, int64_t ninner, int64_t items, int64_t dim_in, int32_t index_bits,
                                  int64_t base, void* d_ptr, void* key_scratch, void* item_scratch, unsigned long long* pinned3,
                                  unsigned long long seq, hipStream_t stream) {
    if (V.capacity < 0 || nouter < 0 || ninner < 0 || items < 0 || (index_bits != 32 && index_bits != 64)) return hipErrorInvalidValue;
    const SubKeys s = sub_carve(key_scratch, nouter, ninner);
    const SubItems it = sub_carve_items(item_scratch, items);
    if (items > 0) {
        const unsigned grid = ex_grid(items, 4);
        if (V.keys.wide) hipLaunchKernelGGL(k_sub_count<true>, dim3(grid), dim3(256), 0, stream, V.keys, V.occ, s, it, nouter, items, dim_in);
        else hipLaunchKernelGGL(k_sub_count<false>, dim3(grid), dim3(256), 0, stream, V.keys, V.occ, s, it, nouter, items, dim_in);
    }
    if (index_bits == 32)
        hipLaunchKernelGGL(k_sub_scan_cells<int32_t>, dim3(1), dim3(EX_SCAN_THREADS), 0, stream, s, it, nouter, items, base,
                           static_cast<int32_t*>(d_ptr), pinned3, seq);
    else
        hipLaunchKernelGGL(k_sub_scan_cells<int64_t>, dim3(1), dim3(EX_SCAN_THREADS), 0, stream, s, it, nouter, items, base,
                           static_cast<int64_t*>(d_ptr), pinned3, seq);
    return hipGetLastError();
}

hipError_t launch_submatrix_emit(const SlotView& V, int64_t nouter, int64_t ninner, int64_t items, int64_t total, int32_t index_bits,
                                 int64_t base, void* d_idx, double* d_vals, void* key_scratch, void* item_scratch,
                                 unsigned long long* pinned2, unsigned long long seq, hipStream_t stream) {
    if (V.capacity < 0 || nouter < 1 || ninner < 1 || items < 1 || total < 1 || (index_bits != 32 && index_bits != 64)) return hipErrorInvalidValue;
    const SubKeys s = sub_carve(key_scratch, nouter, ninner);
    const SubItems it = sub_carve_items(item_scratch, items);
    const SubArgs a{d_idx, d_vals, nouter, items, total, base, pinned2, seq};
    dispatch_wide_it(V.keys.wide, index_bits, [&](auto wide, auto ix) {
        hipLaunchKernelGGL((k_sub_emit<decltype(wide)::value, decltype(ix)>), dim3(ex_grid(items, 4)), dim3(256), 0, stream, V.keys, V.vals,
                           V.occ, s, it, a);
    });
    return hipGetLastError();
}

}  // namespace dsa
