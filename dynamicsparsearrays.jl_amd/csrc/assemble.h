// csrc/assemble.h — launch wrappers and scratch layout of the fold in front of the general write from (row, column, value) triples in
// HBM (dsa_mat_assemble[_dev]), shared by assemble.hip (the kernels) and assemble_host.hip.
#pragma once
#include "dsa_dev.h"
#include "pairsort.h"

namespace dsa {

// ---- the constants a test needs to put runs on the edges of the kernels
constexpr int64_t ASM_TILE = 1024;             // sorted positions per workgroup of the flag, fold and scatter kernels: one lane each, 16 waves
constexpr int ASM_FOLD_INLINE = 64;            // ops of one cell folded by the lane of the run's head; a longer run is finished by a wave
constexpr int ASM_LONG_BLOCKS = 256;           // waves of k_asm_fold_long: each strides over the queue
constexpr int ASM_PIN_WORDS = 2;               // {distinct cells, sequence number}

// a run of more than ASM_FOLD_INLINE ops, as its head's lane leaves it: the fold so far, the next sorted position, the cell's rank
struct AsmLongRun { int64_t next; int64_t rank; double acc; };

// device scratch of one call of n ops (one block on the colmajor orientation)
struct AsmScratch {
    unsigned long long* hdr;                   // [0] runs in the queue [1] the total of the last scan
    PairSort sort; uint32_t* idx; int64_t* k2; int64_t* p2;      // the shared sort and what it leaves, in (column, row, input order)
    uint64_t* words;                           // one flag bit per position: the heads of the sorted ops, then the misses of the folded cells
    uint32_t* tcnt; uint32_t* toff;            // per tile: flags set, their exclusive prefix
    AsmLongRun* queue;
    int64_t* fI; int64_t* fJ; double* fV; uint32_t* flast;       // the folded cells in (column, row) order; flast: input index of the run's last op
    uint8_t* miss;                             // update's mask over the folded cells
    // the compacted misses: they take the place of the sort's buffers, which nothing reads behind the sort
    int64_t* cI; int64_t* cJ; double* cV; uint32_t* clast;
    int64_t tiles, words_n;
};
static inline int64_t asm_tiles(int64_t n) { return (n + ASM_TILE - 1) / ASM_TILE; }
static inline AsmScratch asm_layout(Carver& c, int64_t n) {
    const size_t nn = (size_t)n;
    AsmScratch s;
    s.tiles = asm_tiles(n); s.words_n = (n + 63) / 64;
    s.hdr = c.take<unsigned long long>(256);
    s.sort = pair_sort_layout(c, n);
    s.idx = c.take<uint32_t>(nn * 4);
    s.k2 = c.take<int64_t>(nn * 8);
    s.p2 = c.take<int64_t>(nn * 8);
    s.words = c.take<uint64_t>((size_t)s.words_n * 8);
    s.tcnt = c.take<uint32_t>((size_t)s.tiles * 4);
    s.toff = c.take<uint32_t>((size_t)s.tiles * 4);
    s.queue = c.take<AsmLongRun>((nn / ASM_FOLD_INLINE + 2) * sizeof(AsmLongRun));
    s.fI = c.take<int64_t>(nn * 8);
    s.fJ = c.take<int64_t>(nn * 8);
    s.fV = c.take<double>(nn * 8);
    s.flast = c.take<uint32_t>(nn * 4);
    s.miss = c.take<uint8_t>(nn);
    s.cI = reinterpret_cast<int64_t*>(s.sort.comp[0]);
    s.cJ = reinterpret_cast<int64_t*>(s.sort.comp[1]);
    s.cV = s.sort.pay[0];
    s.clast = reinterpret_cast<uint32_t*>(s.sort.pay[1]);
    return s;
}
static inline size_t assemble_scratch_bytes(int64_t n) { Carver c(nullptr); asm_layout(c, n); return c.bytes(); }
static inline AsmScratch asm_carve(void* base, int64_t n) { Carver c(base); return asm_layout(c, n); }

// The fold, on `stream`, behind the key scan (all keys >= 1; rows in [imin, imin + 2^ibits), columns in [jmin, jmin + 2^jbits)): the
// sort, the heads, their scan — which hands {distinct cells m, seq} to pinned memory — and the fold of every run into fI / fJ / fV /
// flast[0 .. m).  add: the left fold s = V[k1]; s = s + V[k2]; ... in ascending k; otherwise the V of the largest k.  Reads the
// caller's arrays; writes nothing but the scratch and the pinned words.  1 <= n < 2^31.
hipError_t launch_assemble_fold(const int64_t* d_I, const int64_t* d_J, const double* d_V, int64_t n, int64_t imin, int ibits, int64_t jmin,
                                int jbits, bool add, void* scratch, unsigned long long* pinned, unsigned long long seq, hipStream_t stream);
// The compaction, behind launch_assemble_fold and the update's resolve pass on the same stream: the folded cells whose byte in
// s.miss is set, in order, into cI / cJ / cV / clast.  m: the distinct cells of the fold.
hipError_t launch_assemble_compact(void* scratch, int64_t n, int64_t m, hipStream_t stream);

}  // namespace dsa
