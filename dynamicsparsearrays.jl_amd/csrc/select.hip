// csrc/select.hip — K-select: the partitions of a list of outer keys as one compressed matrix (A[:, J] from colmajor, A[I, :] from
// rowmajor), cost proportional to what is selected.
//
// The j-th outer slice of the result is the live partition whose key is sel[j] (any order, repeats allowed; a key without a live
// partition gives an empty slice).  The cells of a partition are the occupied slots strictly between its semaphore and the next live
// semaphore (the end of the slot array behind the last one): its SPAN.  Three launches, two host waits:
//   k_key_spans  one wave per selected key: range check, wave-parallel table search (find_dev.h), the span (tombstoned table entries
//                behind the partition are skipped 64 at a time), cnt[j] = popcount of the span's bitmap words,
//                nchunk[j] = 2048-slot tiles of the slot array the span touches (0 for a span without cells)
//   k_sel_scan   one workgroup: exclusive prefixes of cnt (-> ptr in the caller's index type, and off[] for the emit) and of nchunk
//                (-> the work-item offsets), 8192 keys per step; both totals and the error word go to pinned memory
//   (host: waits for the totals, checks cap and the 32-bit rule, sizes the emit grid from the chunk total)
//   k_sel_emit   one wave per work item (selection j, chunk c): j by an upper-bound search over the chunk prefix, output position =
//                off[j] + occupied slots of the span in front of the chunk (re-popcounted), the chunk's cells compacted by popcount
//                ranks; keys and values loaded and idx / vals stored non-temporally; the last workgroup hands the error word to
//                pinned memory
// No wave owns a whole long partition: a span is cut at the tile boundaries of the slot array, whatever its length.  No atomics on
// the output, no floating-point arithmetic (values are copied bit for bit).  The count phase relies on popcounts only, so every cell
// of a selected partition is delivered; inner-index selection and renumbering (A[I, J] with both lists) is the submatrix export
// (submatrix.hip, dsa_mat_submatrix_compressed[_dev]).  It runs the same work-item pipeline, so what the two have in common is in
// export_dev.h: the span kernel (k_key_spans), the search for the owner of a work item (item_past, item_owner), the part of the span a work item
// covers (span_chunk, chunk_word), the hand-over at the end of a scan (hand_over), the emit grid (ex_grid) and the choice of <WIDE, IT>.
// Bytes in: 8 * nsel selection keys, about 8 * log2(table_len) probed table bytes per key, (kb + 8) per slot of the selected spans,
// their bitmap words twice (count and emit; the emit reads the words in front of a chunk once more to place it: for a span of c
// chunks c / 2 times its bitmap, 1/64 of the slot bytes per pass).  Bytes out: (ib + 8) * total + ib * (nsel + 1).  Nothing is
// proportional to the capacity.
#include "select.h"
#include "export_dev.h"

namespace dsa {

// scratch: four arrays of nsel entries, then the error word and the ticket of the emit (one 8-byte memset)
struct SelScratch {
    int64_t* lo; int64_t* hi;                            // span of selection j: slots [lo, hi), 0-based
    int64_t* off;                                        // cells (k_key_spans), then their exclusive prefix (k_sel_scan)
    int64_t* choff;                                      // chunks, then their exclusive prefix
    uint32_t* err; uint32_t* ticket;
};
static SelScratch sel_carve(void* base, int64_t nsel) {
    SelScratch s;
    s.lo = static_cast<int64_t*>(base);
    s.hi = s.lo + nsel;
    s.off = s.hi + nsel;
    s.choff = s.off + nsel;
    s.err = reinterpret_cast<uint32_t*>(s.choff + nsel);
    s.ticket = s.err + 1;
    return s;
}
size_t select_scratch_bytes(int64_t nsel) { return (size_t)(nsel > 0 ? nsel : 0) * 32 + 8; }

// one workgroup: off / choff become exclusive prefixes in place, ptr[j] = base + off[j], ptr[nsel] = base + total
template <typename IT>
__global__ __launch_bounds__(EX_SCAN_THREADS) void k_sel_scan(SelScratch s, int64_t nsel, int64_t base, IT* __restrict__ ptr,
                                                              unsigned long long* pinned, unsigned long long seq) {
    unsigned long long carry_o, carry_s;
    block_excl_scan2(s.off, s.choff, nsel,
                     [&](int64_t i, unsigned long long ro, unsigned long long rs) {
                         s.off[i] = (int64_t)ro; s.choff[i] = (int64_t)rs; ptr[i] = (IT)(base + (int64_t)ro);
                     },
                     carry_o, carry_s);
    if (threadIdx.x != 0) return;
    ptr[nsel] = (IT)(base + (int64_t)carry_o);
    hand_over(s.err, pinned, seq, 2, carry_o, carry_s);
}

struct SelArgs {
    void* idx; double* val;
    int64_t nsel, items, total, dim_in, base;
    unsigned long long* pinned;         // {error word, sequence number}
    unsigned long long seq;
};

// one wave per work item.  Error bits: 1 an inner key outside 1..dim_in, 2 slots and tables disagree.
template <bool WIDE, typename IT>
__global__ __launch_bounds__(256) void k_sel_emit(KeyArr keys, const double* __restrict__ vals, const uint64_t* __restrict__ occ,
                                                  SelScratch s, SelArgs a) {
    typedef typename std::conditional<WIDE, int64_t, int32_t>::type key_t;
    const key_t* __restrict__ kp = static_cast<const key_t*>(keys.p);
    IT* __restrict__ idx = static_cast<IT*>(a.idx);
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t below = mask_lt(lane);
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    uint32_t err = 0;
    for (int64_t w = (int64_t)blockIdx.x * 4 + wv; w < a.items; w += nwaves) {
        const int64_t j = item_past(s.choff, a.nsel, w, lane) - 1;       // the selection in front of the first whose prefix exceeds w owns it
        if (j < 0 || j >= a.nsel) { err |= 2u; continue; }
        const int64_t lo = s.lo[j], hi = s.hi[j];
        const SpanChunk c = span_chunk(lo, hi, (lo >> EX_TILE_SHIFT) + (w - s.choff[j]));
        if (c.ce <= c.cs) { err |= 2u; continue; }
        int64_t run = s.off[j] + (c.cs > lo ? sel_span_popc(occ, lo, c.cs, lane) : 0);      // output position of the chunk's first cell
        uint32_t nz;
        const uint64_t myword = chunk_word(occ, c, lane, nz);
        for (int q = 0; q < EX_WORDS; q += EX_U) {
            if (((nz >> q) & ((1u << EX_U) - 1u)) == 0u) continue;
            uint64_t wd[EX_U];
            int64_t k[EX_U];
            double v[EX_U];
#pragma unroll
            for (int u = 0; u < EX_U; ++u) {
                wd[u] = readlane64(myword, q + u);
                const int64_t i = ((c.w0 + q + u) << 6) + lane;
                k[u] = -1; v[u] = 0.0;
                if ((wd[u] >> lane) & 1ull) { k[u] = (int64_t)__builtin_nontemporal_load(kp + i); v[u] = __builtin_nontemporal_load(vals + i); }
            }
#pragma unroll
            for (int u = 0; u < EX_U; ++u) {
                if ((wd[u] >> lane) & 1ull) {
                    const int64_t pos = run + popc64(wd[u] & below);
                    if (k[u] == SEM_KEY || pos >= a.total) {
                        err |= 2u;                               // a semaphore inside a span, or more cells than were counted
                    } else {
                        __builtin_nontemporal_store((IT)(k[u] - 1 + a.base), idx + pos);
                        __builtin_nontemporal_store(v[u], a.val + pos);
                        if (k[u] < 1 || k[u] > a.dim_in) err |= 1u;
                    }
                }
                run += popc64(wd[u]);
            }
        }
    }
    emit_epilogue(err, lane, wv, s.err, s.ticket, a.pinned, a.seq);
}

hipError_t launch_select_count(const SlotView& V, const int64_t* d_sel, int64_t nsel, int64_t dim_out, int32_t index_bits, int64_t base,
                               void* d_ptr, void* scratch, unsigned long long* pinned4, unsigned long long seq, hipStream_t stream) {
    if (V.capacity < 0 || V.table_len < 0 || nsel < 0 || nsel > INT32_MAX || (index_bits != 32 && index_bits != 64)) return hipErrorInvalidValue;
    const SelScratch s = sel_carve(scratch, nsel);
    hipError_t e = hipMemsetAsync(s.err, 0, 8, stream);
    if (e != hipSuccess) return e;
    if (nsel > 0)
        hipLaunchKernelGGL(k_key_spans<true>, dim3((unsigned)((nsel + 3) / 4)), dim3(256), 0, stream, V, d_sel, nsel, dim_out, s.lo, s.hi,
                           s.choff, s.off, s.err);
    if (index_bits == 32)
        hipLaunchKernelGGL(k_sel_scan<int32_t>, dim3(1), dim3(EX_SCAN_THREADS), 0, stream, s, nsel, base, static_cast<int32_t*>(d_ptr), pinned4, seq);
    else
        hipLaunchKernelGGL(k_sel_scan<int64_t>, dim3(1), dim3(EX_SCAN_THREADS), 0, stream, s, nsel, base, static_cast<int64_t*>(d_ptr), pinned4, seq);
    return hipGetLastError();
}

hipError_t launch_select_emit(const SlotView& V, int64_t nsel, int64_t items, int64_t total, int64_t dim_in, int32_t index_bits, int64_t base,
                              void* d_idx, double* d_vals, void* scratch, unsigned long long* pinned2, unsigned long long seq,
                              hipStream_t stream) {
    if (V.capacity < 0 || nsel < 1 || items < 1 || total < 1 || (index_bits != 32 && index_bits != 64)) return hipErrorInvalidValue;
    const SelScratch s = sel_carve(scratch, nsel);
    const SelArgs a{d_idx, d_vals, nsel, items, total, dim_in, base, pinned2, seq};
    dispatch_wide_it(V.keys.wide, index_bits, [&](auto wide, auto ix) {
        hipLaunchKernelGGL((k_sel_emit<decltype(wide)::value, decltype(ix)>), dim3(ex_grid(items, 4)), dim3(256), 0, stream, V.keys, V.vals,
                           V.occ, s, a);
    });
    return hipGetLastError();
}

}  // namespace dsa
