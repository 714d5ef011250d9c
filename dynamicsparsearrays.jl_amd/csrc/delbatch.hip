// csrc/delbatch.hip — K-delete-batch: a list of columns (rows) leaves both orientations of a matrix in one device pass
// (dsa_mat_delete_batch[_dev]; the reference's deletecolumn! / deleterow!, src/matrix.jl:95-111, for every key of the list).  In the
// orientation whose partitions the keys name (the OWN one) the listed partitions go away with their semaphores and their table entries
// become tombstones, exactly what deletepartition! leaves (src/pcsr.jl:188-204); in the TWIN every cell whose inner key is listed goes
// away and every semaphore stays.  The kernels only clear occupancy bits: the pack + spread of the survivors is the root rebalance
// the host enqueues behind them (rebalance.hip), so keys and values of cleared slots are never touched.
//
// Five launches on the own stream + two on the twin's, two host waits, whatever n and the partition lengths are:
//   k_sub_hash     (export_dev.h, the kernel of the submatrix export) the list into the open-addressing table: repeats, keys < 1
//   k_del_spans    one wave per key: table lookup (find_dev.h: live_span, the lookup of the exports), the span from the semaphore to
//                  the slot in front of the next live semaphore, its cells by popcount of the bitmap words (one wave step = 64 words =
//                  4096 slots, no per-cell work); a key that is < 1, repeated or without a live partition is recorded with its
//                  index in the list.  Writes lo / hi / table entry per key and adds the cells to a counter (integer atomic)
//   k_del_verdict  one thread: {error word, first bad key, partitions, cells} to pinned memory
//   (host: waits; any error leaves both orientations untouched)
//   k_del_mark_own one wave per key: clears the bits of the span, the semaphore's included.  Two listed partitions may share a bitmap
//                  word: the first and last word of a span take a 64-bit atomicAnd, the words between are plain stores of 0.  Lane 0
//                  writes the tombstone (sems[pos] = 0, live[pos] = 0)
//   k_del_mark_twin streaming, one wave per 512 slots (8 bitmap words) as scale.hip: the keys of the occupied slots are loaded
//                  (non-temporally when the array does not fit the L2) from the 32- or 64-bit array, semaphores (key 0) skipped, the
//                  eight first probes of the table (12 B per entry, <= 48 B per listed key: it stays in the L2) issued before one is
//                  resolved; the hits of a word are a ballot, the word is rewritten by lane 0 — every wave owns its words, no atomics
//                  on the bitmap — and the popcounts go into one integer counter per wave
//   k_del_twin_verdict one thread: the twin's count against the own orientation's (bit 1 of the error word), to pinned memory
// Which bits are cleared depends only on WHETHER a key is in the table, never on where the hash put it, and every count is an integer:
// the result is the same bits from call to call.
// Bytes: own 8 B per key + its span's bitmap words twice; twin occupancy + keys of occupied slots read once = 4.1 B (int32 keys) |
// 8.1 B (int64 keys) per slot + one 8-byte probe per cell (L2) + 8 B per rewritten word.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; no scratch, no LDS in any kernel): k_del_spans 26 VGPRs, 60 SGPRs;
// k_del_mark_own 16 / 32; k_del_mark_twin 55 / 60 in all four instantiations; the two verdict kernels 10 / 18 and 6 / 14.
#include "delbatch.h"
#include "export_dev.h"
#include <type_traits>

namespace dsa {

constexpr int DL_BLOCK = 256;
constexpr int DL_WAVES = DL_BLOCK / 64;
constexpr int DL_WORDS = 8;                               // occupancy words of a span of the twin pass

// scratch: this header, then the key block of export_dev.h with nouter = ninner = n (lo / hi: the span of key j with its semaphore,
// 0-based [lo, hi); choff: its 1-based table entry).  One memset clears the header and the key block's header and key words.
struct DelHeader {
    unsigned long long own_cells;       // cells of the listed partitions (k_del_spans)
    unsigned long long twin_cells;      // cells cleared in the twin (k_del_mark_twin)
    unsigned long long first_bad;       // n - (smallest index of a bad key), 0: none — a maximum, so that 0 is "nothing yet"
    unsigned long long pad[5];
};
static_assert(sizeof(DelHeader) == 64, "the key block behind the header stays 16-byte aligned");

size_t delbatch_scratch_bytes(int64_t n) { return sizeof(DelHeader) + sub_key_block_bytes(n, n); }
static inline SubKeys del_carve(void* scratch, int64_t n) { return sub_carve(static_cast<char*>(scratch) + sizeof(DelHeader), n, n); }

// ---- step 1 ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DL_BLOCK) void k_del_spans(SlotView V, const int64_t* __restrict__ keys, int64_t n, SubKeys s,
                                                        DelHeader* __restrict__ hdr) {
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t j = (int64_t)blockIdx.x * DL_WAVES + wv;
    if (j >= n) return;                                   // whole waves
    const int64_t key = keys[j];
    int64_t bad = -1, lo = 0, hi = 0, pos = 0, cells = 0; // bad: index in the list of the occurrence that is wrong
    uint32_t err = 0;
    if (key < 1) {
        bad = j;
    } else {
        // the table entry of a key holds the index of ONE of its occurrences: every other occurrence is a repeat, and the one that
        // counts as wrong is the later of the two
        uint64_t p = sub_slot(s, key);
        p = sub_resolve(s, key, p, s.tkey[p]);
        const int64_t w = p != SUB_NONE ? (int64_t)s.tpos[p] : j;
        if (w != j) {
            bad = w > j ? w : j;
        } else {
            const KeySpan sp = live_span(V, key, lane);
            if (sp.err) err = 2u;
            else if (sp.pos == 0) bad = j;                // no live partition of this key
            else {
                lo = sp.lo - 1; hi = sp.hi; pos = sp.pos; // with the semaphore: its 1-based slot is the 0-based slot of the first cell
                cells = sp.hi > sp.lo ? sel_span_popc(V.occ, sp.lo, sp.hi, lane) : 0;
            }
        }
    }
    if (lane != 0) return;
    s.lo[j] = lo; s.hi[j] = hi; s.choff[j] = pos;
    if (cells > 0) atomicAdd(&hdr->own_cells, (unsigned long long)cells);
    if (bad >= 0) { err |= 1u; atomicMax(&hdr->first_bad, (unsigned long long)(n - bad)); }
    if (err) atomicOr(s.err, err);
}

// one thread, behind k_sub_hash and k_del_spans on the stream
__global__ void k_del_verdict(const int64_t* __restrict__ keys, int64_t n, SubKeys s, const DelHeader* __restrict__ hdr,
                              unsigned long long* pinned, unsigned long long seq) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    uint32_t e = __hip_atomic_load(s.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    e = ((e & (1u | 4u | 8u)) ? 1u : 0u) | (e & 2u);      // k_sub_hash: 4 a key < 1, 8 a repeat; k_del_spans names the key for both
    const unsigned long long fb = __hip_atomic_load(&hdr->first_bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int64_t bad_key = fb != 0ull && fb <= (unsigned long long)n ? keys[n - (int64_t)fb] : 0;
    const unsigned long long cells = __hip_atomic_load(&hdr->own_cells, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(pinned + 0, (unsigned long long)e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(pinned + 1, (unsigned long long)bad_key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(pinned + 2, (unsigned long long)n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(pinned + 3, cells, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    publish_seq(pinned + 4, seq);
}

// ---- step 2 ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DL_BLOCK) void k_del_mark_own(uint64_t* __restrict__ occ, int64_t* __restrict__ sems, uint8_t* __restrict__ live,
                                                           int64_t n, SubKeys s) {
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t j = (int64_t)blockIdx.x * DL_WAVES + wv;
    if (j >= n) return;
    const int64_t lo = s.lo[j], hi = s.hi[j], pos = s.choff[j];
    if (pos < 1 || hi <= lo || lo < 0) return;            // (step 1 has ruled it out)
    const int64_t w0 = lo >> 6, w1 = (hi - 1) >> 6;
    for (int64_t w = w0 + lane; w <= w1; w += 64) {
        if (w == w0 || w == w1) atomicAnd(reinterpret_cast<unsigned long long*>(occ + w), (unsigned long long)~word_range_mask(w, lo, hi - 1));
        else occ[w] = 0ull;                               // a word between belongs to this span alone
    }
    if (lane == 0) { sems[pos - 1] = 0; live[pos - 1] = 0; }
}

// ---- step 3 ---------------------------------------------------------------------------------------------------------------------
template <bool WIDE, bool NT>
__global__ __launch_bounds__(DL_BLOCK) void k_del_mark_twin(KeyArr keys, uint64_t* __restrict__ occ, int64_t capacity, SubKeys s,
                                                            DelHeader* __restrict__ hdr) {
    typedef typename std::conditional<WIDE, int64_t, int32_t>::type key_t;
    const key_t* __restrict__ kp = static_cast<const key_t*>(keys.p);
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t nwords = (capacity + 63) >> 6;
    const int64_t w0 = ((int64_t)blockIdx.x * DL_WAVES + wv) * DL_WORDS;
    if (w0 >= nwords) return;                             // whole waves: nothing below waits for another wave
    uint64_t ow[DL_WORDS];
#pragma unroll
    for (int j = 0; j < DL_WORDS; ++j) ow[j] = occ[w0 + j < nwords ? w0 + j : nwords - 1];
#pragma unroll
    for (int j = 0; j < DL_WORDS; ++j) ow[j] = w0 + j < nwords ? readfirstlane64(ow[j]) : 0ull;      // words behind the array are empty
    // lane <-> slot: the keys of the occupied slots of the whole span are requested before anything waits
    int64_t k[DL_WORDS];
#pragma unroll
    for (int j = 0; j < DL_WORDS; ++j) {
        k[j] = SEM_KEY;
        if ((ow[j] >> lane) & 1ull) {                     // an occupied slot lies in a word of the array: w0 + j < nwords
            const key_t* src = kp + ((w0 + j) << 6) + lane;
            k[j] = (int64_t)(NT ? __builtin_nontemporal_load(src) : *src);
        }
    }
    // ... and the first probe of every cell before one is resolved (a listed key is >= 1: semaphores and empty slots probe nothing)
    uint64_t p[DL_WORDS];
    int64_t t[DL_WORDS];
#pragma unroll
    for (int j = 0; j < DL_WORDS; ++j) {
        p[j] = 0; t[j] = 0;
        if (k[j] >= 1) { p[j] = sub_slot(s, k[j]); t[j] = s.tkey[p[j]]; }
    }
    unsigned long long cleared = 0;                       // wave-uniform
#pragma unroll
    for (int j = 0; j < DL_WORDS; ++j) {
        const bool hit = k[j] >= 1 && sub_resolve(s, k[j], p[j], t[j]) != SUB_NONE;
        const uint64_t m = __ballot(hit);
        if (m != 0ull) {
            if (lane == 0) occ[w0 + j] = ow[j] & ~m;      // this wave owns the word
            cleared += (unsigned long long)popc64(m);
        }
    }
    if (cleared != 0ull && lane == 0) atomicAdd(&hdr->twin_cells, cleared);
}

// one thread, behind k_del_mark_twin on the twin's stream
__global__ void k_del_twin_verdict(const DelHeader* __restrict__ hdr, unsigned long long expect, unsigned long long* pinned,
                                   unsigned long long seq) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const unsigned long long c = __hip_atomic_load(&hdr->twin_cells, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(pinned + 0, c != expect ? 2ull : 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(pinned + 1, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    publish_seq(pinned + 2, seq);
}

// ---- launch wrappers -----------------------------------------------------------------------------------------------------------
hipError_t launch_delbatch_validate(const SlotView& V, const int64_t* d_keys, int64_t n, void* scratch, unsigned long long* pinned5,
                                    unsigned long long seq, hipStream_t stream) {
    if (V.capacity <= 0 || V.table_len < 0 || n < 1 || n > INT32_MAX || !V.sems || !V.part_keys) return hipErrorInvalidValue;
    const SubKeys s = del_carve(scratch, n);
    DelHeader* hdr = static_cast<DelHeader*>(scratch);
    hipError_t e = hipMemsetAsync(scratch, 0, sizeof(DelHeader) + sub_key_block_clear_bytes(s), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_sub_hash<>, dim3(ex_grid(n, 256)), dim3(256), 0, stream, d_keys, n, INT64_MAX, s);
    hipLaunchKernelGGL(k_del_spans, dim3((unsigned)((n + DL_WAVES - 1) / DL_WAVES)), dim3(DL_BLOCK), 0, stream, V, d_keys, n, s, hdr);
    hipLaunchKernelGGL(k_del_verdict, dim3(1), dim3(64), 0, stream, d_keys, n, s, hdr, pinned5, seq);
    return hipGetLastError();
}

hipError_t launch_delbatch_mark_own(uint64_t* occ, int64_t* sems, uint8_t* live, int64_t n, void* scratch, hipStream_t stream) {
    if (n < 1 || !occ || !sems || !live) return hipErrorInvalidValue;
    const SubKeys s = del_carve(scratch, n);
    hipLaunchKernelGGL(k_del_mark_own, dim3((unsigned)((n + DL_WAVES - 1) / DL_WAVES)), dim3(DL_BLOCK), 0, stream, occ, sems, live, n, s);
    return hipGetLastError();
}

hipError_t launch_delbatch_mark_twin(KeyArr keys, uint64_t* occ, int64_t capacity, int64_t n, bool nt, unsigned long long expect,
                                     void* scratch, unsigned long long* pinned3, unsigned long long seq, hipStream_t stream) {
    if (capacity <= 0 || n < 1) return hipErrorInvalidValue;
    const SubKeys s = del_carve(scratch, n);
    DelHeader* hdr = static_cast<DelHeader*>(scratch);
    const int64_t spans = (((capacity + 63) >> 6) + DL_WORDS - 1) / DL_WORDS;
    const unsigned grid = (unsigned)((spans + DL_WAVES - 1) / DL_WAVES);
#define DSA_DEL_CASE(W_, N_) hipLaunchKernelGGL((k_del_mark_twin<W_, N_>), dim3(grid), dim3(DL_BLOCK), 0, stream, keys, occ, capacity, s, hdr)
    switch ((keys.wide ? 2 : 0) | (nt ? 1 : 0)) {
        case 0: DSA_DEL_CASE(false, false); break;
        case 1: DSA_DEL_CASE(false, true); break;
        case 2: DSA_DEL_CASE(true, false); break;
        default: DSA_DEL_CASE(true, true); break;
    }
#undef DSA_DEL_CASE
    hipLaunchKernelGGL(k_del_twin_verdict, dim3(1), dim3(64), 0, stream, hdr, expect, pinned3, seq);
    return hipGetLastError();
}

}  // namespace dsa
