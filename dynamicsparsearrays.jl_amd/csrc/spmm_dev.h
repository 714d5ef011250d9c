// csrc/spmm_dev.h — what the two dense-block product kernels share (spmm.hip: every partition of an orientation; selprod.hip: the
// partitions of a key list): the per-wave LDS slice, the coalesced load + in-order compaction of nine bitmap words, and the in-order
// walk that sums a row left to right with MM_U loads of X in flight.  Device code only.
#pragma once
#include "wave_dev.h"
#include "find_dev.h"
#include <type_traits>

namespace dsa {

constexpr int MM_BLOCK = 256;
constexpr int MM_WAVES = MM_BLOCK / 64;
constexpr int MM_OWN_WORDS = 8;                          // words of a span
constexpr int MM_LOAD_WORDS = MM_OWN_WORDS + 1;          // ... and the word behind it
constexpr int MM_TILE = MM_WAVES * MM_OWN_WORDS * 64;    // slots per workgroup
constexpr int MM_CELLS = MM_LOAD_WORDS * 64;
constexpr int MM_U = 8;                                  // X loads a lane keeps in flight

template <typename key_t>
struct MmWave {
    double v[MM_CELLS];                  // value of a cell / partition id of a semaphore
    key_t c[MM_CELLS];                   // 0-based row of X, -1: contributes nothing (semaphore, key outside 1..nx)
    uint16_t sem[MM_OWN_WORDS * 64];     // compacted positions of the span's semaphores
};

// Loads words [w0, w0 + 9) of the slot array (clamped to the array) and compacts their occupied slots into S.  Semaphores of the
// first OWN words are listed in S.sem (nsem of them); behind those words the first semaphore ends the compaction (closed = true:
// the open row ends there).  Returns the number of compacted slots.  Executed by one full wave.
// SPAN = true (selprod.hip): the caller knows the slot span [lo, hi) of ONE partition; the words are masked to it and nothing looks
// for semaphores (nsem = 0, closed = false, OWN is not used).
template <bool WIDE, bool NT, int OWN, bool SPAN = false>
__device__ __forceinline__ int mm_load_compact(const typename std::conditional<WIDE, int64_t, int32_t>::type* __restrict__ kp,
                                               const double* __restrict__ vals, const uint64_t* __restrict__ occ, int64_t nwords,
                                               int64_t w0, int64_t nx, MmWave<typename std::conditional<WIDE, int64_t, int32_t>::type>& S,
                                               int lane, int& nsem, bool& closed, int64_t lo = 0, int64_t hi = 0) {
    typedef typename std::conditional<WIDE, int64_t, int32_t>::type key_t;
    uint64_t ow[MM_LOAD_WORDS];
    key_t k[MM_LOAD_WORDS];
    double v[MM_LOAD_WORDS];
#pragma unroll
    for (int j = 0; j < MM_LOAD_WORDS; ++j) ow[j] = occ[w0 + j < nwords ? w0 + j : nwords - 1];
#pragma unroll
    for (int j = 0; j < MM_LOAD_WORDS; ++j) {
        const int64_t w = w0 + j < nwords ? w0 + j : nwords - 1;
        k[j] = NT ? __builtin_nontemporal_load(kp + (w << 6) + lane) : kp[(w << 6) + lane];
    }
#pragma unroll
    for (int j = 0; j < MM_LOAD_WORDS; ++j) {
        const int64_t w = w0 + j < nwords ? w0 + j : nwords - 1;
        v[j] = NT ? __builtin_nontemporal_load(vals + (w << 6) + lane) : vals[(w << 6) + lane];
    }
    const uint64_t unx = (uint64_t)(nx > 0 ? nx : 0);
    const uint32_t nx32 = unx < 0x7fffffffull ? (uint32_t)unx : 0x7fffffffu;
    int n = 0;
    nsem = 0;
    closed = false;
#pragma unroll
    for (int j = 0; j < MM_LOAD_WORDS; ++j) {
        uint64_t o = (closed || w0 + j >= nwords) ? 0ull : readfirstlane64(ow[j]);
        bool issem = false;
        uint64_t sb = 0ull;
        if constexpr (SPAN) {
            o &= word_range_mask(w0 + j, lo, hi - 1);
        } else {
            issem = ((o >> lane) & 1ull) && k[j] == (key_t)SEM_KEY;
            sb = __ballot(issem);
            if (j >= OWN && sb != 0ull) {                    // the open row ends in front of this semaphore
                o &= (sb & (0ull - sb)) - 1ull;
                closed = true;
            }
        }
        if ((o >> lane) & 1ull) {
            const int pos = n + popc64(o & mask_lt(lane));
            const bool ok = WIDE ? (uint64_t)((int64_t)k[j] - 1) < unx : (uint32_t)k[j] - 1u < nx32;      // 1 <= key <= nx
            S.c[pos] = ok ? (key_t)(k[j] - 1) : (key_t)-1;
            S.v[pos] = v[j];
            if (!SPAN && j < OWN && issem) S.sem[nsem + popc64(sb & mask_lt(lane))] = (uint16_t)pos;
        }
        if (!SPAN && j < OWN) nsem += popc64(sb);
        n += popc64(o);
    }
    return n;
}

// sum + the terms of the compacted cells [t0, t1) for this lane's column, in order; MM_U loads of X requested per round
template <typename key_t>
__device__ __forceinline__ double mm_walk(double sum, int t0, int t1, const MmWave<key_t>& S, const double* __restrict__ xcol, int64_t ldx,
                                          bool colok) {
    for (int t = t0; t < t1; t += MM_U) {
        double xv[MM_U], vv[MM_U];
#pragma unroll
        for (int u = 0; u < MM_U; ++u) {
            const bool in = t + u < t1;
            const int tc = in ? t + u : t0;
            const key_t c = S.c[tc];
            const bool ok = in && colok && c >= 0;
            vv[u] = ok ? S.v[tc] : 0.0;
            // straight-line: a lane with nothing to add reads X[0, 0] (nx > 0: it exists) and drops it
            const double xl = xcol[ok ? (int64_t)c * ldx : 0];
            xv[u] = ok ? xl : 0.0;
        }
#pragma unroll
        for (int u = 0; u < MM_U; ++u) {
            // a cell that contributes nothing adds +0.0 * +0.0: a sum that started at +0.0 is never -0.0, so it keeps its bits
            const double p = vv[u] * xv[u];
            sum = sum + p;
        }
    }
    return sum;
}

}  // namespace dsa
