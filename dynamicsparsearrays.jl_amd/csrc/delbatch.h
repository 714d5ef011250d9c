// csrc/delbatch.h — launch wrappers of the batched delete (delbatch.hip), shared with delbatch_host.hip.
#pragma once
#include "dsa_dev.h"

namespace dsa {

// device scratch of a batched delete of n keys: counters, the hash table of the list and three words per key (O(n), nothing
// proportional to the capacity)
size_t delbatch_scratch_bytes(int64_t n);

// Step 1 (k_sub_hash of export_dev.h, k_del_spans, k_del_verdict): writes nothing but the scratch.  Hands
// {error word, first bad key, partitions, cells of the listed partitions (semaphores not counted)} and then `seq` to pinned5[0..4].
// Error word: bit 0 a key that is <= 0, repeated or without a live partition; bit 1 tables out of step with the slots.  n >= 1.
hipError_t launch_delbatch_validate(const SlotView& V, const int64_t* d_keys, int64_t n, void* scratch, unsigned long long* pinned5,
                                    unsigned long long seq, hipStream_t stream);
// Step 2, on the orientation step 1 looked at: clears the occupancy bits of every listed span, its semaphore included, and writes the
// tombstones sems[pos] = 0, live[pos] = 0.
hipError_t launch_delbatch_mark_own(uint64_t* occ, int64_t* sems, uint8_t* live, int64_t n, void* scratch, hipStream_t stream);
// Step 3, on the twin: clears the occupancy bit of every cell whose key is in the table (k_del_mark_twin) and hands
// {error word: bit 1 the count differs from `expect`, cells cleared} and then `seq` to pinned3[0..2].  `stream` is the twin's: the
// caller has waited for step 1.
hipError_t launch_delbatch_mark_twin(KeyArr keys, uint64_t* occ, int64_t capacity, int64_t n, bool nt, unsigned long long expect,
                                     void* scratch, unsigned long long* pinned3, unsigned long long seq, hipStream_t stream);

}  // namespace dsa
