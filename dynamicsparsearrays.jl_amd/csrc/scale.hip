// csrc/scale.hip — the two operations over the stored values as a whole, on gfx950: per-partition reductions
// (dsa_mat_reduce[_dev]: sum, sum |v|, sum v*v, max |v|, count per row / column) and the in-place diagonal scaling
// (dsa_mat_scale[_dev]: v -> ((v * alpha) * r[row]) * c[col]).  Both are one streaming pass over the slot array of an orientation
// and need, for every occupied slot, the partition that owns it: the stored value of the semaphore in front of it (the partition
// id; its key is part_keys[id - 1], as in k_spmm and k_spmv_gather, so tombstones, tables out of key order and pending table entries
// need nothing special).
//
// One wave per span of 512 slots (8 occupancy words), four independent waves per workgroup, no workgroup barrier, no LDS.  A wave
// requests the 8 occupancy words, the 8 x 64 keys (physical width) and the 8 x 64 values of its span, lane <-> slot, coalesced,
// before anything waits, then goes through the words in order.  Inside a word the owner of a slot is the nearest semaphore at or
// below its lane (ballot of key == SEM_KEY, count-leading-zeros of the bits below); in front of the word's first semaphore it is
// the partition that is open, a wave-uniform value carried from word to word.
//
// Reduce (k_reduce + k_reduce_finish) needs NO carry into a span: it never has to know the owner of the cells in front of the
// span's first semaphore.  Per word a segmented inclusive scan over the lanes (6 shuffle steps, a term joins only terms of its own
// partition) gives every partition's total inside the word; the open partition's running total is wave-uniform.  A partition that
// ends inside the span it began in is stored by the wave.  What is left per span is a record of 24 bytes: `head` (the cells in
// front of the first semaphore, the whole span when it has none), `tail` (the cells behind the last semaphore) and the id of the
// tail's partition.  k_reduce_finish, one thread per span that has a semaphore, adds tail + head of the next span + ... up to and
// including the first later span that has a semaphore, left to right, and stores the element.  Every element of the output that
// owns a partition is stored exactly once with a plain store; the order of the additions depends only on the slot layout: no
// floating-point atomics, two calls on one state give the same bits, and a partition may be as long as the array.  The squared term
// is a rounded multiply, the sum a separate add (-ffp-contract=off).  ABSMAX compares the bit patterns of |v| as unsigned 64-bit
// integers: NaN is above Inf, so it propagates like Julia's maximum(abs, ...), and the result is exact in any order.  COUNT adds
// 1.0 per cell (exact below 2^53).  Every accumulator starts at +0.0.
// Bytes: occupancy + keys + values read once = 12.1 B (int32 keys) | 16.1 B (int64 keys) per slot, + 24 B written and read per span
// (0.05 B per slot), + 8 B per output element (the zeroing in front of the launch and the one store).
//
// Scale (k_scale) writes the cells in front of a span's first semaphore too, so it needs their owner: the CARRY comes from a small
// pass in front, the count -> scan -> emit split of compress.hip with the scan operator "last non-empty":
//   k_scale_check  per span: the id stored in its last semaphore (0: none), from the occupancy words and the keys — the values are
//                  not streamed, one value is read per span; the same pass checks every cell key against 1..dim_key;
//   k_scale_tables the key of every live partition against 1..dim_part (16 B per table entry);
//   k_scale_carry  one workgroup: carry[s] = the last non-empty id of the spans in front of s; hands the bounds word to the host.
// The host waits for that word before the first value is written: a stored entry outside size(m) leaves both orientations as they
// were.  k_scale then streams occupancy, keys and values once, gathers f_key[key - 1] per lane and f_part[part_key - 1] per
// semaphore (handed to the partition's lanes by a shuffle), multiplies ((v * alpha) * r) * c — three separately rounded products,
// the same order in both orientations, an absent factor is exactly 1.0 — and stores the VALUES of occupied non-semaphore slots only.
// Keys, occupancy bits, semaphore slots (their value is the partition id) and the tables are never written.
// Bytes: check 4.1 | 8.1 B per slot read + 16 B per span; apply 12.1 | 16.1 B per slot read + 8 B per stored cell written, + the
// factor gathers.  The carry pass costs the second read of the keys; what it buys is that a wave never walks back through a long row.
//
// Slot loads (and the value stores) go around the cache when the slot array does not fit an XCD's L2 beside the vectors (nt).
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; no scratch in any kernel, occupancy 8 waves per SIMD everywhere):
//   k_reduce        int32 keys 46 - 51 VGPRs (ABSMAX 46, COUNT 51), int64 keys 52 - 58; 64 SGPRs; no LDS
//   k_reduce_finish 54 VGPRs (ABSMAX 48), 46 SGPRs, 16 B LDS (the epilogue's error words)
//   k_scale_check   30 VGPRs (int64 keys 24), 69 SGPRs, no LDS
//   k_scale_tables  4 VGPRs, 14 SGPRs, no LDS
//   k_scale_carry   14 VGPRs, 20 SGPRs, 8192 B LDS (one workgroup)
//   k_scale         57 VGPRs, 68 SGPRs, no LDS, in all four instantiations
#include "scale.h"
#include "scale_dev.h"
#include "export_dev.h"
#include <type_traits>

namespace dsa {

// (the span shape SC_*, ScHeader, ScScratch, sc_load_span and the lane helpers are in scale_dev.h: droptol.hip streams the same spans)
constexpr int SC_CARRY_THREADS = 1024;
constexpr int SC_FIN_U = 8;                               // span records k_reduce_finish requests at once
constexpr int64_t SC_NO_SEM = INT64_MIN;                  // span record: the span holds no semaphore

size_t reduce_scratch_bytes(int64_t capacity) { return sizeof(ScHeader) + (size_t)sc_spans(capacity) * 24; }
size_t scale_scratch_bytes(int64_t capacity) { return sizeof(ScHeader) + (size_t)sc_spans(capacity) * 16; }

template <int KIND>
__device__ __forceinline__ double red_term(double v) {
    if (KIND == RED_SUM) return v;
    if (KIND == RED_SQSUM) return v * v;
    if (KIND == RED_COUNT) return 1.0;
    return fabs(v);                                       // ABSSUM, ABSMAX
}
template <int KIND>
__device__ __forceinline__ double red_comb(double a, double b) {
    if (KIND == RED_ABSMAX) return (uint64_t)__double_as_longlong(b) > (uint64_t)__double_as_longlong(a) ? b : a;
    return a + b;
}

// the one store of an output element: partition id -> key -> out[key - 1]
__device__ __forceinline__ void red_store(int64_t id, double x, const int64_t* __restrict__ part_keys, int64_t table_len,
                                          double* __restrict__ out, int64_t n_out, uint32_t& err) {
    if (id < 1 || id > table_len) { err |= 2u; return; }
    const int64_t key = part_keys[id - 1];
    if (key < 1 || key > n_out) { err |= 1u; return; }
    out[key - 1] = x;
}

// ---- reduce --------------------------------------------------------------------------------------------------------------------
template <bool WIDE, bool NT, int KIND>
__global__ __launch_bounds__(SC_BLOCK) void k_reduce(KeyArr keys, const double* __restrict__ vals, const uint64_t* __restrict__ occ,
                                                     int64_t capacity, const int64_t* __restrict__ part_keys, int64_t table_len,
                                                     double* __restrict__ out, int64_t n_out, ScHeader* __restrict__ hdr,
                                                     double* __restrict__ head, double* __restrict__ tail, int64_t* __restrict__ tid) {
    typedef typename std::conditional<WIDE, int64_t, int32_t>::type key_t;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t nwords = (capacity + 63) >> 6;
    const int64_t span = (int64_t)blockIdx.x * SC_WAVES + wv;
    const int64_t w0 = span * SC_WORDS;
    if (w0 >= nwords) return;                             // whole waves: nothing below waits for another wave
    uint64_t ow[SC_WORDS];
    key_t k[SC_WORDS];
    double v[SC_WORDS];
    sc_load_span<WIDE, NT, true>(static_cast<const key_t*>(keys.p), vals, occ, nwords, w0, lane, ow, k, v);

    uint32_t err = 0;
    double acc = 0.0, span_head = 0.0;                    // wave-uniform: total of the open partition so far
    int64_t open_id = 0;
    bool have_sem = false;
#pragma unroll
    for (int j = 0; j < SC_WORDS; ++j) {
        const uint64_t o = ow[j];
        const bool here = (o >> lane) & 1ull;
        const bool issem = here && k[j] == (key_t)SEM_KEY;
        const uint64_t sb = __ballot(issem);
        const uint64_t below = sb & mask_le(lane);
        const int start = below ? top_bit(below) : 0;     // the lane of this lane's semaphore (0: the open partition)
        double x = (here && !issem) ? red_term<KIND>(v[j]) : 0.0;
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {                // segmented inclusive scan: fixed order
            const double y = __shfl_up(x, s, 64);
            if (lane - s >= start) x = red_comb<KIND>(x, y);
        }
        if (sb == 0ull) { acc = red_comb<KIND>(acc, readlane_f64(x, 63)); continue; }
        const int first = __builtin_ctzll(sb), last = top_bit(sb);
        if (first > 0) acc = red_comb<KIND>(acc, readlane_f64(x, first - 1));
        // the open partition ends in front of this word's first semaphore
        if (have_sem) { if (lane == 0) red_store(open_id, acc, part_keys, table_len, out, n_out, err); }
        else span_head = acc;
        have_sem = true;
        // partitions that begin and end inside the word: stored by the lane in front of the next semaphore
        const double idv = __shfl(v[j], start, 64);
        if (below != 0ull && lane < 63 && ((sb >> (lane + 1)) & 1ull)) red_store((int64_t)idv, x, part_keys, table_len, out, n_out, err);
        open_id = (int64_t)readlane_f64(v[j], last);      // partition ids are stored as Float64 (src/pcsr.jl:104)
        acc = readlane_f64(x, 63);                        // the cells behind the last semaphore (+0.0 when it is lane 63)
    }
    if (lane == 0) {
        head[span] = have_sem ? span_head : acc;
        tail[span] = have_sem ? acc : 0.0;
        tid[span] = have_sem ? open_id : SC_NO_SEM;
    }
    if (err) __hip_atomic_fetch_or(&hdr->err, err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// one thread per span that holds a semaphore: the partition open at its end = its tail + the heads of the spans behind it, up to and
// including the first that holds a semaphore, left to right.  SC_FIN_U records are requested per round.
template <int KIND>
__global__ __launch_bounds__(SC_BLOCK) void k_reduce_finish(int64_t nspans, const double* __restrict__ head, const double* __restrict__ tail,
                                                            const int64_t* __restrict__ tid, const int64_t* __restrict__ part_keys,
                                                            int64_t table_len, double* __restrict__ out, int64_t n_out, ScHeader* hdr,
                                                            unsigned long long* pinned, unsigned long long seq) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t s = (int64_t)blockIdx.x * SC_BLOCK + threadIdx.x;
    uint32_t err = 0;
    const int64_t id = s < nspans ? tid[s] : SC_NO_SEM;
    if (id != SC_NO_SEM) {
        double acc = tail[s];
        bool done = false;
        for (int64_t t = s + 1; !done && t < nspans; t += SC_FIN_U) {
            double h[SC_FIN_U];
            int64_t ti[SC_FIN_U];
#pragma unroll
            for (int u = 0; u < SC_FIN_U; ++u) {
                const int64_t q = t + u < nspans ? t + u : nspans - 1;
                h[u] = head[q];
                ti[u] = tid[q];
            }
#pragma unroll
            for (int u = 0; u < SC_FIN_U; ++u) {
                if (!done && t + u < nspans) {
                    acc = red_comb<KIND>(acc, h[u]);
                    done = ti[u] != SC_NO_SEM;
                }
            }
        }
        red_store(id, acc, part_keys, table_len, out, n_out, err);
    }
    emit_epilogue(err, lane, wv, &hdr->err, &hdr->ticket, pinned, seq);
}

// ---- scale ---------------------------------------------------------------------------------------------------------------------
// per span: the id stored in its last semaphore (0: none); every cell key checked against 1..dim_key
template <bool WIDE>
__global__ __launch_bounds__(SC_BLOCK) void k_scale_check(KeyArr keys, const double* __restrict__ vals, const uint64_t* __restrict__ occ,
                                                          int64_t capacity, int64_t dim_key, ScHeader* __restrict__ hdr,
                                                          int64_t* __restrict__ last_id) {
    typedef typename std::conditional<WIDE, int64_t, int32_t>::type key_t;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t nwords = (capacity + 63) >> 6;
    const int64_t span = (int64_t)blockIdx.x * SC_WAVES + wv;
    const int64_t w0 = span * SC_WORDS;
    if (w0 >= nwords) return;
    uint64_t ow[SC_WORDS];
    key_t k[SC_WORDS];
    double unused[SC_WORDS];
    sc_load_span<WIDE, false, false>(static_cast<const key_t*>(keys.p), vals, occ, nwords, w0, lane, ow, k, unused);
    const uint64_t udim = (uint64_t)(dim_key > 0 ? dim_key : 0);
    bool bad = false;
    int64_t last_slot = -1;                               // wave-uniform: 0-based slot of the span's last semaphore
#pragma unroll
    for (int j = 0; j < SC_WORDS; ++j) {
        const bool here = (ow[j] >> lane) & 1ull;
        const bool issem = here && k[j] == (key_t)SEM_KEY;
        const uint64_t sb = __ballot(issem);
        if (here && !issem && !((uint64_t)((int64_t)k[j] - 1) < udim)) bad = true;       // 1 <= key <= dim_key
        if (sb != 0ull) last_slot = ((w0 + j) << 6) + top_bit(sb);
    }
    if (lane == 0) last_id[span] = last_slot >= 0 ? (int64_t)vals[last_slot] : 0;
    if (bad) __hip_atomic_fetch_or(&hdr->err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the key of every live partition (its semaphore is in the slot array) against 1..dim_part
__global__ __launch_bounds__(SC_BLOCK) void k_scale_tables(const int64_t* __restrict__ sems, const int64_t* __restrict__ part_keys,
                                                           int64_t table_len, int64_t dim_part, ScHeader* __restrict__ hdr) {
    const int64_t i = (int64_t)blockIdx.x * SC_BLOCK + threadIdx.x;
    if (i >= table_len || sems[i] == 0) return;
    const int64_t key = part_keys[i];
    if (key < 1 || key > dim_part) __hip_atomic_fetch_or(&hdr->err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// one workgroup: carry[s] = the last non-empty last_id of the spans in front of s (0: none); then the bounds word goes to the host
__global__ __launch_bounds__(SC_CARRY_THREADS) void k_scale_carry(int64_t nspans, const int64_t* __restrict__ last_id,
                                                                  int64_t* __restrict__ carry, ScHeader* hdr, unsigned long long* pinned,
                                                                  unsigned long long seq) {
    __shared__ int64_t sL[SC_CARRY_THREADS];
    const int t = threadIdx.x;
    const int64_t per = (nspans + SC_CARRY_THREADS - 1) / SC_CARRY_THREADS;
    const int64_t a = (int64_t)t * per, b = a + per < nspans ? a + per : nspans;
    int64_t mine = 0;
    for (int64_t s = a; s < b; ++s) { const int64_t id = last_id[s]; if (id != 0) mine = id; }
    sL[t] = mine;
    __syncthreads();
    for (int o = 1; o < SC_CARRY_THREADS; o <<= 1) {      // inclusive scan, operator "the right operand unless it is empty"
        const int64_t left = t >= o ? sL[t - o] : 0;
        __syncthreads();
        if (sL[t] == 0) sL[t] = left;
        __syncthreads();
    }
    int64_t run = t > 0 ? sL[t - 1] : 0;
    for (int64_t s = a; s < b; ++s) {
        carry[s] = run;
        const int64_t id = last_id[s];
        if (id != 0) run = id;
    }
    if (t != 0) return;
    // k_scale_check and k_scale_tables are complete: this launch is behind them on the stream
    const uint32_t e = __hip_atomic_load(&hdr->err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(pinned + 0, (unsigned long long)e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    publish_seq(pinned + 1, seq);
}

// f_part[part_key(id) - 1], or 1.0 when the factor is absent or the id / key is not usable (the check pass has ruled that out)
__device__ __forceinline__ double sc_part_factor(int64_t id, const int64_t* __restrict__ part_keys, int64_t table_len,
                                                 const double* __restrict__ f_part, int64_t dim_part) {
    if (f_part == nullptr || id < 1 || id > table_len) return 1.0;
    const int64_t key = part_keys[id - 1];
    return key >= 1 && key <= dim_part ? f_part[key - 1] : 1.0;
}

template <bool WIDE, bool NT>
__global__ __launch_bounds__(SC_BLOCK) void k_scale(KeyArr keys, double* __restrict__ vals, const uint64_t* __restrict__ occ, int64_t capacity,
                                                    const int64_t* __restrict__ part_keys, int64_t table_len, double alpha,
                                                    const double* __restrict__ f_key, int64_t dim_key, const double* __restrict__ f_part,
                                                    int64_t dim_part, int key_is_row, const int64_t* __restrict__ carry) {
    typedef typename std::conditional<WIDE, int64_t, int32_t>::type key_t;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t nwords = (capacity + 63) >> 6;
    const int64_t span = (int64_t)blockIdx.x * SC_WAVES + wv;
    const int64_t w0 = span * SC_WORDS;
    if (w0 >= nwords) return;
    uint64_t ow[SC_WORDS];
    key_t k[SC_WORDS];
    double v[SC_WORDS];
    sc_load_span<WIDE, NT, true>(static_cast<const key_t*>(keys.p), vals, occ, nwords, w0, lane, ow, k, v);
    const uint64_t udim = (uint64_t)(dim_key > 0 ? dim_key : 0);
    double open_f = sc_part_factor(carry[span], part_keys, table_len, f_part, dim_part);      // wave-uniform: the open partition's factor

    // the gathers of the whole span are requested before the first product waits for one
    double fk[SC_WORDS], fs[SC_WORDS];
    bool cell[SC_WORDS];
    uint64_t sbs[SC_WORDS];
#pragma unroll
    for (int j = 0; j < SC_WORDS; ++j) {
        const bool here = (ow[j] >> lane) & 1ull;
        const bool issem = here && k[j] == (key_t)SEM_KEY;
        sbs[j] = __ballot(issem);
        cell[j] = here && !issem && (uint64_t)((int64_t)k[j] - 1) < udim;
        fk[j] = (cell[j] && f_key != nullptr) ? f_key[(int64_t)k[j] - 1] : 1.0;
        fs[j] = issem ? sc_part_factor((int64_t)v[j], part_keys, table_len, f_part, dim_part) : 1.0;
    }
#pragma unroll
    for (int j = 0; j < SC_WORDS; ++j) {
        const uint64_t sb = sbs[j];
        const uint64_t below = sb & mask_le(lane);
        const double fl = __shfl(fs[j], below ? top_bit(below) : 0, 64);
        const double fp = below ? fl : open_f;
        const double r = key_is_row ? fk[j] : fp, c = key_is_row ? fp : fk[j];
        double x = v[j] * alpha;
        x = x * r;
        x = x * c;
        if (cell[j]) {
            double* dst = vals + ((w0 + j) << 6) + lane;      // a cell lies in a word of the array: w0 + j < nwords
            if (NT) __builtin_nontemporal_store(x, dst); else *dst = x;
        }
        if (sb != 0ull) open_f = readlane_f64(fs[j], top_bit(sb));
    }
}

// ---- launch wrappers -----------------------------------------------------------------------------------------------------------
template <bool WIDE, bool NT>
static void launch_reduce_kind(unsigned grid, hipStream_t stream, int32_t kind, const SlotView& V, double* out, int64_t n_out, const ScScratch& S) {
#define DSA_RED_CASE(K_) hipLaunchKernelGGL((k_reduce<WIDE, NT, K_>), dim3(grid), dim3(SC_BLOCK), 0, stream, V.keys, V.vals, V.occ, V.capacity, V.part_keys, \
                                            V.table_len, out, n_out, S.hdr, static_cast<double*>(S.a0), static_cast<double*>(S.a1), static_cast<int64_t*>(S.a2))
    switch (kind) {
        case RED_SUM: DSA_RED_CASE(RED_SUM); break;
        case RED_ABSSUM: DSA_RED_CASE(RED_ABSSUM); break;
        case RED_SQSUM: DSA_RED_CASE(RED_SQSUM); break;
        case RED_ABSMAX: DSA_RED_CASE(RED_ABSMAX); break;
        default: DSA_RED_CASE(RED_COUNT); break;
    }
#undef DSA_RED_CASE
}

hipError_t launch_reduce(const SlotView& V, int32_t kind, double* out, int64_t n_out, bool nt, void* scratch, unsigned long long* pinned,
                         unsigned long long seq, hipStream_t stream) {
    if (V.capacity <= 0 || kind < RED_SUM || kind > RED_COUNT) return hipErrorInvalidValue;
    const ScScratch S(scratch, V.capacity);
    hipError_t e = hipMemsetAsync(S.hdr, 0, sizeof(ScHeader), stream);
    if (e != hipSuccess) return e;
    const unsigned grid = (unsigned)((S.nspans + SC_WAVES - 1) / SC_WAVES);
    switch ((V.keys.wide ? 2 : 0) | (nt ? 1 : 0)) {
        case 0: launch_reduce_kind<false, false>(grid, stream, kind, V, out, n_out, S); break;
        case 1: launch_reduce_kind<false, true>(grid, stream, kind, V, out, n_out, S); break;
        case 2: launch_reduce_kind<true, false>(grid, stream, kind, V, out, n_out, S); break;
        default: launch_reduce_kind<true, true>(grid, stream, kind, V, out, n_out, S); break;
    }
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const unsigned fgrid = (unsigned)((S.nspans + SC_BLOCK - 1) / SC_BLOCK);
#define DSA_FIN_CASE(K_) hipLaunchKernelGGL((k_reduce_finish<K_>), dim3(fgrid), dim3(SC_BLOCK), 0, stream, S.nspans, static_cast<const double*>(S.a0), \
                                            static_cast<const double*>(S.a1), static_cast<const int64_t*>(S.a2), V.part_keys, V.table_len, out, n_out, S.hdr, pinned, seq)
    if (kind == RED_ABSMAX) DSA_FIN_CASE(RED_ABSMAX); else DSA_FIN_CASE(RED_SUM);      // every other kind combines with +
#undef DSA_FIN_CASE
    return hipGetLastError();
}

hipError_t launch_scale_check(const SlotView& V, int64_t dim_key, int64_t dim_part, void* scratch, unsigned long long* pinned,
                              unsigned long long seq, hipStream_t stream) {
    if (V.capacity <= 0) return hipErrorInvalidValue;
    const ScScratch S(scratch, V.capacity);
    hipError_t e = hipMemsetAsync(S.hdr, 0, sizeof(ScHeader), stream);
    if (e != hipSuccess) return e;
    const unsigned grid = (unsigned)((S.nspans + SC_WAVES - 1) / SC_WAVES);
    int64_t* open_at = static_cast<int64_t*>(S.a0);
    if (V.keys.wide) hipLaunchKernelGGL((k_scale_check<true>), dim3(grid), dim3(SC_BLOCK), 0, stream, V.keys, V.vals, V.occ, V.capacity, dim_key, S.hdr, open_at);
    else hipLaunchKernelGGL((k_scale_check<false>), dim3(grid), dim3(SC_BLOCK), 0, stream, V.keys, V.vals, V.occ, V.capacity, dim_key, S.hdr, open_at);
    if (V.table_len > 0)
        hipLaunchKernelGGL(k_scale_tables, dim3((unsigned)((V.table_len + SC_BLOCK - 1) / SC_BLOCK)), dim3(SC_BLOCK), 0, stream, V.sems, V.part_keys,
                           V.table_len, dim_part, S.hdr);
    hipLaunchKernelGGL(k_scale_carry, dim3(1), dim3(SC_CARRY_THREADS), 0, stream, S.nspans, static_cast<const int64_t*>(S.a0), static_cast<int64_t*>(S.a1),
                       S.hdr, pinned, seq);
    return hipGetLastError();
}

hipError_t launch_scale_apply(KeyArr keys, double* vals, const uint64_t* occ, int64_t capacity, const int64_t* part_keys, int64_t table_len,
                              double alpha, const double* f_key, int64_t dim_key, const double* f_part, int64_t dim_part, bool key_is_row,
                              bool nt, const void* scratch, hipStream_t stream) {
    if (capacity <= 0) return hipErrorInvalidValue;
    const ScScratch S(const_cast<void*>(scratch), capacity);
    const unsigned grid = (unsigned)((S.nspans + SC_WAVES - 1) / SC_WAVES);
    const int64_t* carry = static_cast<const int64_t*>(S.a1);
#define DSA_SCALE_CASE(W_, N_) hipLaunchKernelGGL((k_scale<W_, N_>), dim3(grid), dim3(SC_BLOCK), 0, stream, keys, vals, occ, capacity, part_keys, table_len, \
                                                  alpha, f_key, dim_key, f_part, dim_part, key_is_row ? 1 : 0, carry)
    switch ((keys.wide ? 2 : 0) | (nt ? 1 : 0)) {
        case 0: DSA_SCALE_CASE(false, false); break;
        case 1: DSA_SCALE_CASE(false, true); break;
        case 2: DSA_SCALE_CASE(true, false); break;
        default: DSA_SCALE_CASE(true, true); break;
    }
#undef DSA_SCALE_CASE
    return hipGetLastError();
}

}  // namespace dsa
