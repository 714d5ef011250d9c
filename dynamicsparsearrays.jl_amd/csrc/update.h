// csrc/update.h — launch wrappers of the in-place value update addressed by (row, column) triples in HBM and of the batched read
// that stays in HBM (dsa_mat_update_values[_dev], dsa_mat_get_batch_dev), shared by update.hip (the kernels) and update_host.hip.
#pragma once
#include "dsa_dev.h"

namespace dsa {

// ---- the constants a test needs to put ops on the edges of the kernels and to build collisions in the claim table
constexpr int UPD_BLOCK = 256;                 // ops per workgroup of the locate, claim and apply kernels: one lane per op, 4 waves of 64
constexpr int UPD_RESOLVE_BLOCKS = 1024;       // workgroups of the resolve kernel at most: beyond it a wave strides over several 64-op groups
constexpr int UPD_K_BITS = 32;                 // a claim word is (slot << UPD_K_BITS) | k: slot = 1-based colmajor slot, k = op index
// The claim table: upd_table_cap(n) 64-bit words, the power of two >= 2 * n (at least 2; load <= 1/2), zeroed by a memset; 0 = empty.
// The first bucket of a slot is (slot * 0x9E3779B97F4A7C15 mod 2^64) >> (64 - log2(cap)) — Fibonacci hashing, the function of the key
// tables of export_dev.h (fib_bucket) — and a probe moves on by one bucket, wrapping at the end.
static inline uint64_t upd_table_cap(int64_t n) {
    uint64_t c = 2;
    while (c < 2 * (uint64_t)(n > 0 ? n : 0)) c <<= 1;
    return c;
}

// what a located op holds instead of a slot when it has none
constexpr int64_t UPD_MISS = 0;                // no live partition, an empty one, or no cell with the inner key
constexpr int64_t UPD_ZERO_KEY = -1;           // I[k] == 0 or J[k] == 0: the semaphore's key, never looked up
constexpr int64_t UPD_BROKEN = -2;             // a live table entry without a semaphore: tables out of step with the slots

// error bits of the verdict (pinned[0])
constexpr unsigned UPD_E_ZERO = 1u, UPD_E_BROKEN = 2u, UPD_E_MISS = 4u, UPD_E_DUP = 8u;
constexpr int UPD_PIN_WORDS = 8;               // {error bits, first zero-key op, first broken / disagreeing op, first missing op, first
                                               //  duplicate op, missing ops, winning ops, sequence number}

// device scratch of one call of n ops.  The colmajor block: the records of the resolve waves, the claim table, the slots, the
// winner flags; the rowmajor block: its slots.
constexpr int UPD_REC_WORDS = 6;               // per resolve wave: missing ops, winning ops, then the first op (or INT64_MAX) that has a
                                               // zero key, is broken or disagrees, is missing, lost its claim
struct UpdScratch {
    int64_t* rec; unsigned long long* table; uint64_t tmask; int tshift;      // colmajor block only
    int64_t* slots; uint8_t* win;                                             // win: colmajor block only
};
static inline size_t upd_rec_bytes() { return (size_t)UPD_RESOLVE_BLOCKS * (UPD_BLOCK / 64) * UPD_REC_WORDS * sizeof(int64_t); }
static inline UpdScratch upd_carve(void* base, int64_t n, bool colmajor) {
    UpdScratch s{nullptr, nullptr, 0, 0, nullptr, nullptr};
    char* p = static_cast<char*>(base);
    if (colmajor) {
        const uint64_t cap = upd_table_cap(n);
        s.rec = reinterpret_cast<int64_t*>(p);
        s.table = reinterpret_cast<unsigned long long*>(p + upd_rec_bytes());
        s.tmask = cap - 1;
        s.tshift = 64 - __builtin_ctzll(cap);
        p += upd_rec_bytes() + (size_t)cap * 8;
    }
    s.slots = reinterpret_cast<int64_t*>(p);
    if (colmajor) s.win = reinterpret_cast<uint8_t*>(s.slots + n);
    return s;
}
static inline size_t update_scratch_bytes(int64_t n, bool colmajor) {
    return (colmajor ? upd_rec_bytes() + (size_t)upd_table_cap(n) * 8 + (size_t)n : 0) + (size_t)n * 8 + 16;
}

// Locate (k_upd_locate, on the orientation's stream): slots[k] = the 1-based slot of the cell (key[k], part[k]) of this orientation —
// the lookup of dsa_mat_get_batch: live partition part[k], inner key key[k] — or UPD_MISS / UPD_ZERO_KEY / UPD_BROKEN.  With
// `colmajor` the claim table is cleared in front and every located op claims its slot in the same kernel.  Writes nothing but the
// scratch.  At most 2^UPD_K_BITS - 1 ops per call and slots per orientation (hipErrorInvalidValue beyond: the host checks first).
hipError_t launch_update_locate(const SlotView& V, const int64_t* d_key, const int64_t* d_part, int64_t n, void* scratch, bool colmajor,
                                hipStream_t stream);
// Resolve + verdict (k_upd_resolve, k_upd_verdict; on the colmajor stream, behind both locates): win[k] = 1 iff op k is located and
// holds the claim of its slot (the largest k that addresses it); d_missing[k] (may be nullptr) = 1 iff op k has no slot.  `strict`: a
// missing op is an error; `add`: a located op that lost its claim is.  Hands UPD_PIN_WORDS words to pinned memory.
hipError_t launch_update_resolve(int64_t n, void* col_scratch, const void* row_scratch, bool strict, bool add, uint8_t* d_missing,
                                 unsigned long long* pinned, unsigned long long seq, hipStream_t stream);
// Apply (k_upd_apply, on the orientation's stream, after the host has seen no error): the winners store V[k] (add: vals + V[k]) into
// vals[slots[k] - 1]; a slot outside the array or one whose key is the semaphore's is never written.
hipError_t launch_update_apply(KeyArr keys, double* vals, int64_t capacity, const double* d_V, int64_t n, const int64_t* slots,
                               const uint8_t* win, bool add, hipStream_t stream);
// out[k] = the stored value of (key[k], part[k]) or +0.0; found[k] (may be nullptr) = 1 iff the cell is stored.  No scratch, no wait.
hipError_t launch_get_batch_dev(const SlotView& V, const int64_t* d_key, const int64_t* d_part, int64_t n, double* d_out, uint8_t* d_found,
                                hipStream_t stream);

}  // namespace dsa
