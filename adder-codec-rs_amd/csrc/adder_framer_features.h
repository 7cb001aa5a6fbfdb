// adder_framer_features.h -- shared between the feature-detection kernels of the framer and the framer C-ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/adder_framer.h"
#include "adder_framer_features.hpp"
#include "adder_framer_kernels.h"

namespace adder {

// per-call scratch, n = events of the call
struct FramerFeatureScratch {
    uint32_t *keys0, *keys1, *idx0, *idx1;  // [n] unit keys and input indices, double-buffered for the radix sort
    uint8_t *val8_sorted;                   // [n] val8 of the event at sorted position j
    uint8_t *val8_input;                    // [n] the same at input index i (the candidate's own centre)
    uint32_t *t_after;                      // [n] by input index
    uint8_t *mark;                          // [n] 1 = feature
    uint32_t *offs;                         // [n] exclusive scan of mark
    uint2 *runs;                            // [n_units] {begin, end} of the unit's run in sorted order, {0, 0}: none
    void *temp;
    size_t temp_bytes;
};

// what persists in the context
struct FramerFeatureState {
    uint8_t *plane;           // [h][w][c] running_intensities
    uint32_t *carry;          // {valid, t} of the last event ingested with detection on
    AdderFramerFeature *out;  // features of the call, stream order
    uint64_t out_cap;
    uint32_t *count;          // their number
};

size_t framer_features_temp_bytes(uint64_t n);

// events ev[0, n) (3 dwords each) in stream order: framing (as adder_framer_launch_segment does it) and detection
hipError_t framer_features_run(const uint32_t *ev, uint64_t n, uint64_t index_base, const FramerArgs &a,
                               uint32_t key_bits, const FramerFeatureScratch &s, const FramerFeatureState &st,
                               hipStream_t stream);

}  // namespace adder
