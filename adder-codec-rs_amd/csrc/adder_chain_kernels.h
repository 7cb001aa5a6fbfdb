// adder_chain_kernels.h -- the part of a camera source's push that adder_prophesee.hip and adder_davis.hip share
// (adder_chain.hip): sort the records' (key, index) pairs, scan their step counts, place their steps.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/adder_hip.h"

namespace adder {

struct ChainScratch {  // per push, for `cap` records (adder_source_util.hpp reserves and frees it)
    uint32_t *keys0, *keys1, *idx0, *idx1;
    uint32_t *cnt;            // steps of the record (0..2)
    uint32_t *offs;           // exclusive scan of cnt
    AdderSparseStep *stage;   // two step slots per record
    void *temp;               // hipcub's, chain_temp_bytes(cap, the source's plane)
    size_t temp_bytes;
    uint64_t cap;
};

// blocks of 256 lanes for n items
inline uint32_t grid_of(uint64_t n) { return (uint32_t)((n + 255u) / 256u); }

// what the sort and the scan of n_records take at most, and a scan over n_plane (0: the source has none)
size_t chain_temp_bytes(uint64_t n_records, uint32_t n_plane);
// sorts (keys0, idx0) by the low `bits` bits of the key, stable; the result ends in keys0 / idx0
hipError_t chain_sort_pairs(const ChainScratch &s, uint64_t n, int bits, hipStream_t stream);
// offs = exclusive sum of cnt over n entries, in s.temp (the source's own count arrays go through here too)
hipError_t chain_exclusive_sum(const ChainScratch &s, const uint32_t *cnt, uint32_t *offs, uint64_t n,
                               hipStream_t stream);
// s.offs = exclusive sum of s.cnt, then *total_dst (device) = the steps of all n records; n > 0
hipError_t chain_scan_counts(const ChainScratch &s, uint64_t n, unsigned long long *total_dst, hipStream_t stream);
// record i's s.cnt[i] steps from its two slots to d_steps + s.offs[i]
hipError_t chain_scatter(const ChainScratch &s, uint64_t n, AdderSparseStep *d_steps, hipStream_t stream);

}  // namespace adder
