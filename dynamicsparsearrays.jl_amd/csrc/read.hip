// csrc/read.hip — the read paths of one structure: batched getindex (k_get_batch, k_get_small), the device-side invariant
// checker (k_check_slots, k_check_table) and the view of one partition (k_partition_range, k_view_small).  None of them writes a
// slot or a table; each sees the structure through a SlotView (dsa_dev.h) and finds a partition's slots with find_dev.h.  Their host
// side is the "read paths" part of pma_host.hip.
#include "find_dev.h"

namespace dsa {

// ---- batched read-only lookups -----------------------------------------------------------------------
// getindex(pma,key) src/pma.jl:189-193 ; getindex(pcsc,key,partition) src/pcsr.jl:222-232 ;
// getindex(mpcsc,row,col) src/pcsr.jl:261-267.  One lane per query; each lane replays the reference's bisection.
// one lookup by one lane; *err receives E_BOUNDS / E_ASSERT (0: none)
__device__ double get_one(int mode, const SlotView& V, int64_t key, int64_t qb, int32_t* err) {
    int64_t from = 1, to = V.capacity;
    if (mode != 0) {
        int64_t partition = qb;
        if (mode == 2) {
            const DFoundKey f = d_find_table(V.part_keys, V.part_live, V.table_len, qb);
            if (!(f.has && f.key == qb)) return 0.0;
            partition = f.pos;
        }
        if (partition < 1 || partition > V.table_len) { *err = E_BOUNDS; return 0.0; }
        const PartSpan sp = part_span(V, partition);
        if (sp.err) { *err = sp.err; return 0.0; }        // _pos_of_partition_start @assert
        from = sp.from; to = sp.to;
    }
    const DFound f = d_find(V.keys, V.vals, V.occ, key, from, to);
    return (f.has && f.key == key) ? f.val : 0.0;
}
__global__ void k_get_batch(int mode, SlotView V, const int64_t* qa, const int64_t* qb, int64_t n, double* out, int32_t* err_out) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    int32_t err = 0;
    out[i] = get_one(mode, V, qa[i], mode != 0 ? qb[i] : 0, &err);
    if (err) atomicCAS(err_out, 0, err);
}
// Up to 64 lookups without a copy command: the queries are read from, and the answers written to, a pinned landing area of the handle —
// io[0..63] keys, io[64..127] partitions / columns, io[128..191] answers, io[192] first error, io[193] the sequence number the host polls
// for.  A scalar getindex (A[i, j], v[k]) is one launch and a poll: ~15 us instead of ~70 (two uploads, a memset, two downloads into pageable
// memory, a stream synchronisation).
__global__ __launch_bounds__(64) void k_get_small(int mode, SlotView V, int64_t* io, int n, unsigned long long seq) {
    const int lane = threadIdx.x;
    int32_t err = 0;
    if (lane < n) {
        const int64_t key = __hip_atomic_load(io + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        const int64_t qb = mode != 0 ? __hip_atomic_load(io + 64 + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : 0;
        const double v = get_one(mode, V, key, qb, &err);
        __hip_atomic_store(io + 128 + lane, __double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    const uint64_t eb = __ballot(err != 0);
    const int first = eb ? __ffsll((unsigned long long)eb) - 1 : 0;
    const int32_t e0 = __shfl(err, first, 64);
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) {
        __hip_atomic_store(io + 192, (int64_t)(eb ? e0 : 0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        publish_seq(reinterpret_cast<unsigned long long*>(io) + 193, seq);
    }
}
hipError_t launch_get_small(int mode, const SlotView& V, int64_t* io, int n, unsigned long long seq, hipStream_t stream) {
    hipLaunchKernelGGL(k_get_small, dim3(1), dim3(64), 0, stream, mode, V, io, n, seq);
    return hipGetLastError();
}

hipError_t launch_get_batch(int mode, const SlotView& V, const int64_t* qa, const int64_t* qb, int64_t n, double* out, int32_t* err_out,
                            hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    const int block = 64;
    hipLaunchKernelGGL(k_get_batch, dim3((unsigned)((n + block - 1) / block)), dim3(block), 0, stream, mode, V, qa, qb, n, out, err_out);
    return hipGetLastError();
}

// ---- device-side invariant checker (the structural checks of the reference's test/utils.jl:68-113, at full size) ------
// report[0] = occupied cells, [1] = semaphore cells, [2] = semaphore cells whose table entry does not point back,
// [3] = key-order violations inside a partition (or anywhere, for a plain vector), [4] = live table entries that do not
// point at a semaphore cell holding their id, [5] = occupancy bits at or beyond the capacity
__global__ void k_check_slots(KeyArr keys, const double* vals, const uint64_t* occ, int64_t capacity, int64_t occ_words,
                              const int64_t* sems, int64_t table_len, unsigned long long* report) {
    const int64_t s0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;      // 0-based slot
    unsigned long long n_occ = 0, n_sem = 0, bad_sem = 0, bad_order = 0;
    if (s0 < capacity && ((occ[s0 >> 6] >> (s0 & 63)) & 1ull)) {
        n_occ = 1;
        const int64_t k = keys[s0];
        if (sems != nullptr && k == SEM_KEY) {
            n_sem = 1;
            const int64_t id = (int64_t)vals[s0];
            if (id < 1 || id > table_len || sems[id - 1] != s0 + 1) bad_sem = 1;
        } else {
            const int64_t p = d_prev_occupied(occ, s0, 1);                  // previous occupied position (1-based), 0 if none
            if (p >= 1) {
                const int64_t pk = keys[p - 1];
                const bool prev_is_sem = sems != nullptr && pk == SEM_KEY;
                if (!prev_is_sem && !(pk < k)) bad_order = 1;
            }
        }
    }
    unsigned long long beyond = 0;
    const int64_t w = s0;                                                   // reuse the grid for the words past the capacity
    if (w < occ_words && (w << 6) >= capacity) beyond = (unsigned long long)popc64(occ[w]);
    else if (w < occ_words && ((w + 1) << 6) > capacity) beyond = (unsigned long long)popc64(occ[w] & ~mask_lt((int)(capacity & 63)));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        n_occ += __shfl_xor(n_occ, o, 64); n_sem += __shfl_xor(n_sem, o, 64); bad_sem += __shfl_xor(bad_sem, o, 64);
        bad_order += __shfl_xor(bad_order, o, 64); beyond += __shfl_xor(beyond, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (n_occ) atomicAdd(&report[0], n_occ);
        if (n_sem) atomicAdd(&report[1], n_sem);
        if (bad_sem) atomicAdd(&report[2], bad_sem);
        if (bad_order) atomicAdd(&report[3], bad_order);
        if (beyond) atomicAdd(&report[5], beyond);
    }
}
__global__ void k_check_table(KeyArr keys, const double* vals, const uint64_t* occ, int64_t capacity, const int64_t* sems,
                              const int64_t* col_keys, const uint8_t* col_live, int64_t table_len, unsigned long long* report) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= table_len) return;
    const int64_t pos = sems[i];
    bool bad = false;
    if (pos != 0) {
        if (pos < 1 || pos > capacity || !occ_test(occ, pos) || keys[pos - 1] != SEM_KEY || vals[pos - 1] != (double)(i + 1)) bad = true;
        if (col_live != nullptr && !col_live[i]) bad = true;
        if (col_live != nullptr && i > 0) {                                  // live column keys ascend with the id
            int64_t j = i - 1;
            while (j >= 0 && !col_live[j]) --j;
            if (j >= 0 && !(col_keys[j] < col_keys[i])) bad = true;
        }
    } else if (col_live != nullptr && col_live[i]) bad = true;
    if (bad) atomicAdd(&report[4], 1ull);
}
hipError_t launch_check(const SlotView& V, int64_t occ_words, unsigned long long* report, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(report, 0, 8 * sizeof(unsigned long long), stream);
    if (e != hipSuccess) return e;
    const int64_t n = V.capacity > occ_words ? V.capacity : occ_words;
    hipLaunchKernelGGL(k_check_slots, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, V.keys, V.vals, V.occ, V.capacity, occ_words,
                       V.sems, V.table_len, report);
    if (V.sems != nullptr && V.table_len > 0)
        hipLaunchKernelGGL(k_check_table, dim3((unsigned)((V.table_len + 255) / 256)), dim3(256), 0, stream, V.keys, V.vals, V.occ, V.capacity,
                           V.sems, V.part_keys, V.part_live, V.table_len, report);
    return hipGetLastError();
}

// view(mpcsc, :, col)  src/views.jl:15-35 : slot range of the column
__global__ void k_partition_range(SlotView V, int64_t col, int64_t* out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    out[0] = 0; out[1] = 0; out[2] = 0;
    const DFoundKey f = d_find_table(V.part_keys, V.part_live, V.table_len, col);
    if (!(f.has && f.key == col)) return;
    const PartSpan sp = part_span(V, f.pos);
    if (sp.err) { out[2] = sp.err; return; }
    out[0] = sp.from + 1;
    out[1] = sp.to;
    out[3] = f.pos;
}
// view(mpcsc, :, col) (src/views.jl:15-35) in ONE launch for partitions of up to VIEW_SMALL_SLOTS slots: partition lookup, then the
// occupied cells of its slot range packed in slot order into out_k / out_v.  meta[0] = from, meta[1] = to, meta[2] = error code,
// meta[3] = partition id, meta[4] = number of cells or -1 when the range is longer (the caller then takes the general K-pack path),
// meta[5] = key of the last cell packed (host word [6]).  Column views, slices and deletecolumn! / deleterow! need one host round trip
// this way.  One workgroup of VIEW_BLOCK threads (round 6; one wave until then: a 10 000-cell column took 115 us of dependent word after
// word): (1) every thread counts its share of the occupancy words, all loads in flight at once; (2) exclusive prefix per word in LDS;
// (3) the waves take the words round-robin, lane <-> slot, and store rank-addressed — coalesced reads, independent of each other.
constexpr int VIEW_BLOCK = 1024;
constexpr int VIEW_WORDS = (int)(VIEW_SMALL_SLOTS / 64) + 1;          // a range of VIEW_SMALL_SLOTS slots touches at most this many words
__global__ __launch_bounds__(VIEW_BLOCK) void k_view_small(SlotView V, int64_t col, KeyArr out_k, double* __restrict__ out_v,
                                                           int64_t out_cap, int64_t* meta, int64_t* host, int64_t host_cells,
                                                           unsigned long long seq, int64_t range_from, int64_t range_to) {
    // host (pinned, may be null): [0..4] the meta words, [5] the sequence number the host polls for, [6] the last key, then host_cells
    // keys and host_cells values — the first cells of the view go straight to the host with the meta words: one launch and no copy
    // command for a short column (a D2H copy into the caller's pageable vectors + a stream synchronisation cost 60 us per view; 20 us this way)
    __shared__ uint64_t sMask[VIEW_WORDS];
    __shared__ uint32_t sPref[VIEW_WORDS];
    __shared__ uint32_t sWave[VIEW_BLOCK / 64];
    __shared__ int64_t sLast;
    const KeyArr keys = V.keys;
    const double* __restrict__ vals = V.vals;
    const uint64_t* __restrict__ occ = V.occ;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t from = 0, to = 0, err = 0, pid = 0;
    // range_from > 0: no partition lookup, the stored cells of the slot range [range_from, range_to] (iteration over a small vector,
    // src/pma.jl:165-180: the same one-launch hand-over as a column view).  The lookup is executed by every wave (uniform result).
    DFoundKey f{0, 0, false};
    if (range_from > 0) { from = range_from; to = range_to; }
    else f = d_find_table_fast(V.part_keys, V.part_live, V.table_len, col);
    if (range_from <= 0 && f.has && f.key == col) {
        const PartSpan sp = part_span(V, f.pos);
        if (sp.err) err = sp.err;
        else { from = sp.from + 1; to = sp.to; pid = f.pos; }
    }
    int64_t cnt = 0;
    if (threadIdx.x == 0) sLast = 0;
    if (from != 0 && to >= from) {
        if (to - from + 1 > VIEW_SMALL_SLOTS) cnt = -1;
        else {
            const int64_t lo0 = from - 1, hi0 = to - 1;
            const int64_t w0 = lo0 >> 6;
            const int nw = (int)((hi0 >> 6) - w0) + 1;                      // <= VIEW_WORDS
            const int per = (nw + VIEW_BLOCK - 1) / VIEW_BLOCK;             // words per thread, contiguous
            const int t0 = threadIdx.x * per;
            uint32_t mine = 0;
            for (int q = t0; q < t0 + per && q < nw; ++q) {
                const uint64_t m = occ[w0 + q] & word_range_mask(w0 + q, lo0, hi0);
                sMask[q] = m;
                mine += (uint32_t)popc64(m);
            }
            // exclusive scan of the per-thread counts: inside the wave by shuffles, across the waves through LDS
            uint32_t inc = mine;
            for (int o = 1; o < 64; o <<= 1) { const uint32_t y = __shfl_up(inc, o, 64); if (lane >= o) inc += y; }
            if (lane == 63) sWave[wave] = inc;
            __syncthreads();
            uint32_t base = 0, total = 0;
            for (int v = 0; v < VIEW_BLOCK / 64; ++v) { const uint32_t c = sWave[v]; if (v < wave) base += c; total += c; }
            uint32_t run = base + inc - mine;
            for (int q = t0; q < t0 + per && q < nw; ++q) { sPref[q] = run; run += (uint32_t)popc64(sMask[q]); }
            __syncthreads();
            cnt = (int64_t)total;
            if (cnt > out_cap) cnt = -1;
            else {
                // four words per wave and step: the loads of all four are in flight before the first store (the stores may alias the
                // loads as far as the compiler knows: word after word, every iteration waited for its own loads — 35 us for 366 words)
                constexpr int NWAVES = VIEW_BLOCK / 64, U = 4;
                for (int q0 = wave; q0 < nw; q0 += NWAVES * U) {
                    int64_t kk[U]; double vv[U]; int64_t r[U]; bool on[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int q = q0 + u * NWAVES;
                        on[u] = false; r[u] = 0; kk[u] = 0; vv[u] = 0.0;
                        if (q < nw) {
                            const uint64_t mask = sMask[q];
                            if ((mask >> lane) & 1ull) {
                                on[u] = true;
                                r[u] = (int64_t)sPref[q] + popc64(mask & mask_lt(lane));
                                const int64_t slot = ((w0 + q) << 6) + lane;
                                kk[u] = keys[slot]; vv[u] = vals[slot];
                            }
                        }
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        if (!on[u]) continue;
                        out_k[r[u]] = kk[u]; out_v[r[u]] = vv[u];
                        if (r[u] == cnt - 1) sLast = kk[u];
                        if (host != nullptr && r[u] < host_cells) {
                            __hip_atomic_store(host + 8 + r[u], kk[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                            __hip_atomic_store(host + 8 + host_cells + r[u], __double_as_longlong(vv[u]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                        }
                    }
                }
            }
        }
    }
    __builtin_amdgcn_s_waitcnt(0);                     // every lane's cells have left
    __syncthreads();
    if (threadIdx.x == 0) {
        const int64_t last_key = cnt > 0 ? sLast : 0;
        meta[0] = from; meta[1] = to; meta[2] = err; meta[3] = pid; meta[4] = cnt; meta[5] = last_key;
        if (host != nullptr) {
            const int64_t m5[5] = {from, to, err, pid, cnt};
            for (int q = 0; q < 5; ++q) __hip_atomic_store(host + q, m5[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(host + 6, last_key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            publish_seq(reinterpret_cast<unsigned long long*>(host) + 5, seq);
        }
    }
}
hipError_t launch_view_small(const SlotView& V, int64_t col, KeyArr out_k, double* out_v, int64_t out_cap, int64_t* meta, int64_t* host,
                             int64_t host_cells, unsigned long long seq, int64_t range_from, int64_t range_to, hipStream_t stream) {
    hipLaunchKernelGGL(k_view_small, dim3(1), dim3(VIEW_BLOCK), 0, stream, V, col, out_k, out_v, out_cap, meta, host, host_cells, seq,
                       range_from, range_to);
    return hipGetLastError();
}

hipError_t launch_partition_range(const SlotView& V, int64_t col, int64_t* out, hipStream_t stream) {
    hipLaunchKernelGGL(k_partition_range, dim3(1), dim3(64), 0, stream, V, col, out);
    return hipGetLastError();
}

}  // namespace dsa
