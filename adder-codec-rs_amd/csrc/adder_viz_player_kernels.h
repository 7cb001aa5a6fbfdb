// adder_viz_player_kernels.h -- between adder_viz_player_api.cpp and adder_viz_player.hip (include/adder_viz_player.h
// is the public side).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/adder_framer.h"  // AdderFramerFeature
#include "adder_framer.hpp"

namespace adder {

enum : uint32_t { kVizStatusRange = 1u, kVizStatusDepth = 2u };

struct VizScalars {  // device words of one call, read back once the schedule is known
    unsigned long long bad;  // smallest index of an event outside the plane (UINT64_MAX: none)
    unsigned long long eof;  // index of the first EOF / undecodable wire record (n: none)
    uint32_t status;         // kVizStatus*
    uint32_t n_pops, overflow;
    int32_t w_end, m_end;
    uint32_t n_feat;  // features of the call (detection on)
};

struct VizArgs {
    uint32_t width, height, channels, units, row_units;
    uint32_t unit_bits, row_bits;  // radix bits of the two keys; key == units / height: takes part in nothing
    uint32_t ring;
    FramerConsts k;
    // carried state
    FramerPx *px;        // units
    uint8_t *ring_val;   // ring * units: pending values, slot = frame % ring
    uint8_t *ring_some;  // ring * units: their Some mask (late drops leave holes)
    uint8_t *running;    // units: running_frame
    uint32_t *cnt;       // height * ring: in-time fills per (row, pending frame)
    uint8_t *done;       // height: chunk_filled_tracker
    uint32_t *run_lo;    // units + 1: where each unit's run starts in the call's unit order
};

struct VizScratch {  // per call; n entries unless said otherwise
    uint32_t *ukeys0, *ukeys1, *uidx0, *uidx1;  // unit order
    uint32_t *rkeys0, *rkeys1, *ridx0, *ridx1;  // row order
    int32_t *s_l;      // unit order: the unit's last_filled after the event
    uint8_t *s_val;    // unit order: its last intensity after the event
    FramerPx *s_px;    // unit order, at run heads: the unit's state after its last event that counts
    int32_t *l_in;     // input order: L of a checked event, -1 otherwise
    int32_t *pm;       // its inclusive prefix maximum
    unsigned long long *comb_in, *comb;  // row order: (row << 32 | L + 1) and its inclusive maximum
    uint32_t *cnt_call;  // height * ring
    int32_t *nat_call;   // height * ring
    uint8_t *done_new;   // height
    int32_t *pops;       // ring + 1
    uint8_t *flushed;    // ring + 1
    void *temp;
    size_t temp_bytes;
    VizScalars *sc;
    const uint32_t *ukeys, *uidx, *rkeys, *ridx;  // the sorted arrays, set by viz_prepare
};

// Feature detection (adder_viz_player_features.hpp): what a call made with detection on adds.  Null plane: off.
struct VizDetect {
    uint8_t *plane;               // carried running_intensities [height][width][channels]
    uint32_t carry_valid, carry_t;  // the carried last event
    uint64_t index_base;          // global index of the call's first event
    // per call, n entries, input order
    uint8_t *val_in;              // the unit's u8 value after the event
    uint32_t *t_after;            // the t ingest_event_for_chunk left in the event
    uint8_t *mark;                // FAST candidates that are corners
    uint32_t *flag, *offs;        // ... that are not the first event of a period, and their exclusive sum
    AdderFramerFeature *feat;     // the features, in stream order
    int32_t *feat_w;              // frames_written of the period each one lies in
};

size_t viz_temp_bytes(uint64_t n);
// n <= INT32_MAX - 1.  Queues keys, both sorts, the walk, coverage, the scans and the schedule on `stream`.  The caller
// reads VizScalars, pops and flushed afterwards.  Changes no carried state.
// With det.plane set it also queues the walk's detection arm, the candidates and, behind the schedule, the features
// with their periods (det.feat, det.feat_w, VizScalars::n_feat).
hipError_t viz_prepare(const VizArgs &a, int source, const void *d_in, uint64_t n, int32_t w0, int32_t m0, int has_limit,
                       uint32_t limit, int opening, int finish, VizScratch &s, const VizDetect &det, hipStream_t stream);
// Writes the call's n_pops frames in `form`, then commits: running frame, pending ring, counts, trackers, unit state.
// stamps: the call's n_stamps cross stamps (viz_stamp_key, sorted; device memory), painted into the running frame.
// With det.plane set the plane is committed too.
hipError_t viz_handout_commit(const VizArgs &a, uint64_t n, uint64_t lim, int32_t w0, uint32_t n_pops, int form,
                              uint8_t *d_frames, const VizScratch &s, const unsigned long long *stamps, uint32_t n_stamps,
                              const VizDetect &det, hipStream_t stream);

}  // namespace adder
