// adder_davis_kernels.h -- between adder_davis_api.cpp and adder_davis.hip (include/adder_davis.h is the public side).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/adder_davis.h"
#include "adder_chain_kernels.h"

namespace adder {

struct DavisScalars {  // device words of one push, read back once
    unsigned long long bad;        // smallest index of an event outside the plane, `before` first (UINT64_MAX: none)
    unsigned long long bad_frame;  // smallest pixel whose frame value is refused (UINT64_MAX: none)
    unsigned long long ev_steps;   // steps of the two event lists
    unsigned long long gap_steps;  // steps of the frame gaps
};

struct DavisArgs {
    uint32_t width, height, units;
    uint32_t chunk_h;   // height / 4
    uint32_t key_bits;  // radix bits of a pixel key; key `units` marks an event that makes no step
    int32_t mode;
    uint32_t tps, ref_time;
};

struct DavisPlanes {  // the camera state per pixel
    int64_t *ts;
    double *ln;
};

struct DavisPacket {  // one push
    double c;
    int64_t start, end;      // as step 1 leaves them (RawDvs: end = start + 1)
    int64_t end_of_last;     // the second check of the held events
    int32_t held_check2;     // 1: the held events must have t > end_of_last; 0: no second check (RawDvs)
    const AdderDavisEvent *held, *before, *after;  // device
    uint64_t n_held, n_before, n_after;
    const double *frame;     // device, [h][w]
};

struct DavisWalkEvent {  // an event as the walk reads it: its pixel's events side by side, in step order
    int64_t t;
    uint32_t rank;   // its step rank: where its count and its two step slots are
    uint32_t flags;  // bit 0: on; bit 1: the last event of its pixel
};

struct DavisScratch {
    ChainScratch chain;       // for chain.cap list events (held + before); cnt, offs and stage by step rank
    uint32_t *order;          // chain.cap: step rank -> list index (held events first)
    DavisWalkEvent *sorted;   // chain.cap: by pixel, then step rank
    uint32_t *gcnt, *goffs;   // by pixel: gap steps (0 or 1), their exclusive scan
    AdderSparseStep *gstage;  // by pixel
    DavisScalars *sc;
};

// One packet on the `work` planes (a copy of the committed ones, made by the caller): checks, the two lists' steps,
// the gaps, the frame.  d_steps receives ev_steps + gap_steps + units steps in the raw modes (room: 2 * (n_held +
// n_before) + 2 * units); Framed only writes d_img (units bytes) and the planes.  The caller reads s.sc afterwards.
hipError_t davis_generate(const DavisArgs &a, const DavisPacket &pk, const DavisPlanes &work, const DavisScratch &s,
                          AdderSparseStep *d_steps, uint8_t *d_img, hipStream_t stream);
// end of input: one ADDER_SPARSE_FLUSH step per pixel in raster order
hipError_t davis_flush_steps(const DavisArgs &a, AdderSparseStep *d_steps, hipStream_t stream);

}  // namespace adder
