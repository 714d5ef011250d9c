// csrc/insert.h — launch wrappers and scratch layout of the batched insert of cells that are not stored yet, from (row, column, value)
// triples in HBM (dsa_mat_insert_batch[_dev]), shared by insert.hip (the kernels) and insert_host.hip.
#pragma once
#include "dsa_dev.h"
#include "pairsort.h"

namespace dsa {

// ---- the constants a test needs to put ops and runs on the edges of the kernels
constexpr int INS_BLOCK = 256;                 // ops per workgroup of the locate, offset and place kernels: one lane per sorted op
constexpr int INS_TILE_WORDS = 8;              // occupancy words of a tile of the rank and merge passes: the span of scale.hip (SC_WORDS)
constexpr int64_t INS_TILE = INS_TILE_WORDS * 64;      // slots of a tile: one wave each

// what a sorted op holds in kind[]
constexpr uint8_t INS_SKIP = 0;                // already stored (an error without DSA_INS_SKIP_EXISTING) or refused: contributes nothing
constexpr uint8_t INS_CELL = 1;                // one new cell behind its predecessor slot
constexpr uint8_t INS_HEAD = 2;                // the first cell of a new partition: its semaphore goes in front of it (two items)

// error bits of the verdict (pinned[0])
constexpr unsigned INS_E_DUP = 1u, INS_E_EXISTS = 2u, INS_E_MIDDLE = 4u, INS_E_BROKEN = 8u;
constexpr int INS_PIN_WORDS = 10;              // {error bits, first (later) duplicate op, first stored op, first op of a partition in the middle
                                               //  of the table, first op of a broken partition, stored ops, items, new partitions, cells in
                                               //  the array, sequence number}
constexpr int INS_REC_WORDS = 6;               // per locate workgroup: stored ops, new partitions, then the smallest op index (INT64_MAX:
                                               // none) that is a duplicate, stored, in the middle, broken

// device scratch of one orientation for a call of n ops on an array of `capacity` slots
struct InsScratch {
    // the shared sort (build.hip: launch_pair_sort) and what it leaves: input index, inner key and partition key in (partition, key) order
    PairSort sort; uint32_t* idx; int64_t* key; int64_t* part;
    int64_t* pred;                             // 1-based predecessor slot of a sorted op (0: in front of everything), the op's own slot when stored
    uint8_t* kind;                             // INS_SKIP / INS_CELL / INS_HEAD per sorted op
    uint64_t* off;                             // n + 1 exclusive prefixes, per sorted op and the totals: items (low 32 bits), new partitions (high 32 bits)
    uint64_t* bsum;                            // per locate workgroup: the sums of the same two, then their exclusive prefixes
    int64_t* rec;                              // INS_REC_WORDS per locate workgroup
    uint32_t* tcnt; int64_t* toff;             // per tile: occupied slots, their exclusive prefix
    int64_t* hdr;                              // [0] the last occupied slot of the array (0: none) [1] the cells in the array
    int64_t nblocks, tiles;
};
static inline int64_t ins_blocks(int64_t n) { return (n + INS_BLOCK - 1) / INS_BLOCK; }
static inline int64_t ins_tiles(int64_t capacity) { return capacity > 0 ? (capacity + INS_TILE - 1) / INS_TILE : 1; }
static inline size_t ins_up(size_t b) { return (b + 255) & ~(size_t)255; }
static inline size_t insert_scratch_bytes(int64_t n, int64_t capacity) {
    const size_t nn = (size_t)n, nb = (size_t)ins_blocks(n), nt = (size_t)ins_tiles(capacity);
    return pair_sort_bytes(n) + ins_up(nn * 4) + 3 * ins_up(nn * 8) + ins_up((nn + 1) * 8) + ins_up(nn) + ins_up(nb * 8) + ins_up(nb * INS_REC_WORDS * 8) + ins_up(nt * 4) +
           ins_up(nt * 8) + 256;
}
static inline InsScratch ins_carve(void* base, int64_t n, int64_t capacity) {
    InsScratch s;
    char* q = static_cast<char*>(base);
    auto take = [&q](size_t b) { char* r = q; q += ins_up(b); return r; };
    const size_t nn = (size_t)n;
    s.nblocks = ins_blocks(n); s.tiles = ins_tiles(capacity);
    s.hdr = reinterpret_cast<int64_t*>(take(256));
    s.sort = pair_sort_carve(take(pair_sort_bytes(n)), n);
    s.idx = reinterpret_cast<uint32_t*>(take(nn * 4));
    s.key = reinterpret_cast<int64_t*>(take(nn * 8));
    s.part = reinterpret_cast<int64_t*>(take(nn * 8));
    s.pred = reinterpret_cast<int64_t*>(take(nn * 8));
    s.off = reinterpret_cast<uint64_t*>(take((nn + 1) * 8));
    s.kind = reinterpret_cast<uint8_t*>(take(nn));
    s.bsum = reinterpret_cast<uint64_t*>(take((size_t)s.nblocks * 8));
    s.rec = reinterpret_cast<int64_t*>(take((size_t)s.nblocks * INS_REC_WORDS * 8));
    s.tcnt = reinterpret_cast<uint32_t*>(take((size_t)s.tiles * 4));
    s.toff = reinterpret_cast<int64_t*>(take((size_t)s.tiles * 8));
    return s;
}

// Everything in front of the first write, on the orientation's stream (V: its view; part / key: the partition and inner keys of the
// ops — columns and rows for colmajor — all >= 1, with the value ranges [pmin, pmin + 2^pbits) and [kmin, kmin + 2^kbits)):
// the sort, the last occupied slot, the locate pass, the verdict (records reduced, block sums scanned, INS_PIN_WORDS words to pinned
// memory), the offsets, and the tile counts of the array with their scan.  d_existing (may be nullptr) gets 1 for a stored op, 0 for
// the others, by input index.  Writes nothing but the scratch, the pinned words and d_existing.
hipError_t launch_insert_prepare(const SlotView& V, const int64_t* d_part, const int64_t* d_key, int64_t n, int64_t pmin, int pbits,
                                 int64_t kmin, int kbits, void* scratch, uint8_t* d_existing, unsigned long long* pinned,
                                 unsigned long long seq, hipStream_t stream);
// The merge, behind launch_insert_prepare of the same arguments once the host has seen no error: every old cell and every new item
// stored at the slot the spread of `m` cells over dst_cap slots gives its rank, the dst_cap / 64 occupancy words of the destination
// written whole from the spread's geometry (m = old cells + items: every rank has its writer), sems[id - 1] rewritten for every semaphore moved or created, part_keys /
// part_live written for the new partitions (ids table_len + 1 ...).  table_entries = table_len + new partitions: no table is written
// beyond it.
hipError_t launch_insert_merge(const SlotView& V, const double* d_val, int64_t n, void* scratch, KeyArr dst_keys, double* dst_vals,
                               uint64_t* dst_occ, int64_t dst_cap, int64_t m, int64_t* sems, int64_t* part_keys, uint8_t* part_live,
                               int64_t table_entries, hipStream_t stream);

}  // namespace dsa
