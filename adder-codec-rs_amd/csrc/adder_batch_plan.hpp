// adder_batch_plan.hpp -- which kernels a batch of frames runs (enqueue_frames), as a pure function of the context's
// and the batch's facts: no HIP, no environment.  tests/test_batch_plan.py drives it on the CPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "adder_variant.hpp"

namespace adder {

// What the compaction scratch ring is laid out for (alloc_scratch): fixed slots per segment and frame (lean records,
// Continuous staging), or one record log per segment and chunk (per-event records of the generic / bounded Collapse
// kernels: log_capacity).
enum ScratchKind : uint32_t { kScratchNone, kScratchLean, kScratchLean8, kScratchCont, kScratchLog2, kScratchLog3 };

struct BatchPlanIn {
    // the context
    uint32_t multi_mode, time_mode, channels;  // ADDER_MULTI_*, ADDER_TIME_*
    uint32_t delta_t_max, dtm_max_seen, ref_time;
    uint32_t c_thresh, c_thresh_max;
    uint32_t n_units, max_depth;
    uint32_t launch_depth;                      // frames per frame-kernel launch (1 while running intensities are on)
    uint8_t continuous, generic_sticky, perpx;
    uint8_t needs_perpx;                        // feature mode that adjusts c_thresh per unit, or a region of interest
    uint8_t feature_path;                       // feature detection or a region of interest
    uint8_t cr_valid, frac_time_seen;
    float cr_time;
    uint64_t frames_done, run_bound;
    uint8_t records_only, wire_batch;           // the batch hands its records out / writes the raw sink's records
    // what the running-intensities side plane shows while it is on (ADDER_VIEW_*); 0 with the plane off and in the
    // Intensity view.  D, DeltaT and SAE need the root's best event in full and last_fired_t in both time modes: only the
    // generic and the Continuous frame kernels have a view instantiation (kVarView) -- no other kernel may be chosen
    uint8_t side_view;
    // the batch
    uint32_t num_frames;
    float time_spanned;
    // test switches (ADDER_HIP_NO_LP / _LR / _RR / _CR): the next kernel down DESIGN §4.1's table
    uint8_t no_lp, no_lr, no_rr, no_cr;
};

struct BatchPlan {
    uint32_t variant;
    ScratchKind scratch;     // what the ring must hold (kScratchNone: as it is -- Continuous)
    uint32_t lean;           // BatchArgs::base.lean
    uint8_t cr_valid, frac_time_seen;  // the context's new values
    float cr_time;
    uint8_t generic_sticky;  // set once the batch has been queued
    const char *refused;     // not null: the batch is refused (a caller's mistake), nothing to queue
};

// Pixels deeper than one fired level cannot occur when Collapse pops the root as soon as it has accumulated once
// (delta_t_max <= time_spanned): then the lean step (adder_pixel.hpp lean_step) runs.  Once a generic batch has run,
// pixels may hold deeper arenas (or a root that the lean step's "time_spanned >= delta_t_max" folding does not
// describe), so the choice is sticky until adder_hip_reset: update_quality_manual can lower delta_t_max mid-stream
// (video.rs:1264-1287).
inline bool lean_possible(const BatchPlanIn &in) {
    return !in.generic_sticky && !in.perpx && !in.needs_perpx && !in.side_view && in.multi_mode == ADDER_MULTI_COLLAPSE &&
           (float)in.delta_t_max <= in.time_spanned;
}

// The most events one frame can emit: the lean step at most 3 per unit (root event, Collapse filler, pop_top's
// event); the generic step its whole arena (<= max_depth levels) plus pop_top's event.
inline size_t worst_case_events_per_frame(const BatchPlanIn &in) {
    if (in.continuous) return (size_t)in.n_units * (in.max_depth + 3u);
    return (size_t)in.n_units * (lean_possible(in) ? 3u : in.max_depth + 1u);
}

// The bounded Collapse step (adder_pixel.hpp cb_step): Collapse with delta_t_max > time_spanned, a uniform c_thresh,
// and every sum its prefix coordinates form an exact integer below 2^24 -- integer time_spanned, at most delta_t_max /
// time + 1 frames of 8-bit intensities before the pop.  rr_possible: its conditions without the mode; pop_at_once_ok:
// delta_t_max <= time_spanned is fine too -- Mode Normal, where a new root is then popped in the frame it starts
// (adder_pixel.hpp kRrFlushPop).
inline bool rr_possible(const BatchPlanIn &in, bool frac_time_seen, bool pop_at_once_ok) {
    const float T = in.time_spanned;
    if (in.continuous || in.perpx || in.needs_perpx || in.side_view || frac_time_seen) return false;
    const double dtm = (double)(in.delta_t_max > in.dtm_max_seen ? in.delta_t_max : in.dtm_max_seen);
    if (!((float)in.delta_t_max > T) && !pop_at_once_ok) return false;
    if (!(T >= 1.0f) || T != (float)(uint32_t)T || T > 65536.0f) return false;
    if (dtm + 2.0 * T >= 8388608.0) return false;
    if ((dtm / T + 3.0) * 255.0 >= 8388608.0) return false;
    return true;
}
inline bool cb_possible(const BatchPlanIn &in) {
    return in.multi_mode == ADDER_MULTI_COLLAPSE && rr_possible(in, in.frac_time_seen, false);
}

inline BatchPlan plan_batch(const BatchPlanIn &in) {
    BatchPlan p{};
    const float T = in.time_spanned;
    const bool collapse = in.multi_mode == ADDER_MULTI_COLLAPSE, abs_t = in.time_mode == ADDER_TIME_ABSOLUTE_T;
    const bool generic = !in.continuous && !lean_possible(in);
    const bool cb = generic && cb_possible(in);  // the bounded Collapse step instead of the generic one
    const bool frac = in.frac_time_seen || !(T >= 1.0f) || T != (float)(uint32_t)T;
    // constant runs: c_thresh is 0 now and cannot grow (c_thresh_max 0: crf 0), the time step is the one of every batch
    // since the reset.  Once lost, the property stays lost until adder_hip_reset (a rolled-back batch included).
    const bool cr_valid = in.cr_valid && !(in.c_thresh != 0 || in.c_thresh_max != 0 || frac || in.feature_path || in.perpx ||
                                           (in.cr_time != 0.0f && in.cr_time != T));
    const bool cr = cb && cr_valid && !in.no_cr;  // ... then only the roots are stepped (adder_cr_kernel)
    // how long a run can be by now: frames since the reset in AbsoluteT (last_fired_t / T is an integer of that size), in
    // DeltaT the bound the kernels' own reports keep down (AdderHipCtx::run_bound)
    // (a batch that hands its records to the multi-GPU gather takes the bound every rank shares -- the frames since the
    // reset: the kernels' reports follow each band's own content, a static band would leave the integer-state kernel where
    // a busy one stays, and root expands ONE record kind per chunk)
    const uint64_t run_frames = (abs_t || in.records_only) ? in.frames_done
                                                           : (in.run_bound < in.frames_done ? in.run_bound : in.frames_done);
    // rho * 255 and rho * time_spanned stay exact in binary32 for every run length rho of the batch
    const bool runs_exact = (double)(run_frames + in.num_frames) * (T > 255.0f ? (double)T : 255.0) < 16777216.0;
    // AbsoluteT: last_fired_t / T rides along as an integer when time_spanned == ref_time >= 255
    const bool abs_t_integer = T == (float)in.ref_time && in.ref_time >= 255u;
    // run records (adder_rr_kernel): the same regime with integer state (Mode Normal under the same conditions runs it
    // too -- adder_pixel.hpp rr_step; the other two kernels are Collapse's)
    const bool rr_regime = cr || (generic && !collapse && cr_valid && rr_possible(in, frac, true));
    const bool rr = rr_regime && !in.no_rr && (!abs_t || abs_t_integer) && runs_exact;
    // lean runs (adder_lr_kernel): the lean regime in DeltaT under the same property, in blocked batches (batches that
    // hand their records out -- the multi-GPU gather -- run it too: the {rho, word} records are the smallest payload)
    const bool lr_time = in.time_mode == ADDER_TIME_DELTA_T || (abs_t && abs_t_integer);
    const bool lr = !generic && !in.continuous && collapse && lr_time && cr_valid && !in.no_lr && in.launch_depth > 1u &&
                    in.num_frames > 1u && runs_exact;
    // ... in packed bytes (adder_lp_kernel, four units per lane): DeltaT batches whose records the expansion reads itself
    // (the pair's records lie in one run: batch_park_layout keeps a pair of segments adjacent)
    const bool lp = lr && !in.no_lp && in.time_mode == ADDER_TIME_DELTA_T && !in.records_only;
    p.variant = (lp ? kVarPacked : 0u) | ((lp && in.channels == 3) ? kVarPackedRgb : 0u) | (collapse ? kVarCollapse : 0u) |
                (abs_t ? kVarAbsT : 0u) | (generic ? kVarGeneric : 0u) | (in.continuous ? kVarContinuous : 0u) |
                (in.n_units >= 4u ? kVarWide : 0u) | (cb ? kVarBounded : 0u) | (cr ? kVarConstRuns : 0u) |
                (lr ? kVarLeanRuns : 0u) | (rr ? kVarRunRecords : 0u) | (in.wire_batch ? kVarWire : 0u) |
                ((in.records_only && !lr) ? kVarLeanLog : 0u) | (in.side_view ? kVarView : 0u);
    // per-event records go to a log per segment and chunk, sized by the hard bound of what a segment can emit (pop_top and
    // a flush exclude each other in one frame when delta_t_max >= 2 * time: 2 instead of 3 per frame); lean records are
    // 12 bytes in AbsoluteT, 8 otherwise (adder_pixel.hpp lean_decode8)
    p.scratch = in.continuous ? kScratchNone
              : generic ? ((collapse && (double)in.delta_t_max >= 2.0 * (double)T) ? kScratchLog2 : kScratchLog3)
              : abs_t ? kScratchLean : kScratchLean8;
    // 2: lean-runs records (lr_decode8), 3: run records (rr_event)
    p.lean = rr ? 3u : (generic || in.continuous) ? 0u : lr ? 2u : 1u;
    p.cr_valid = cr_valid;
    p.cr_time = T;
    p.frac_time_seen = frac;
    p.generic_sticky = in.generic_sticky || generic;
    if (in.wire_batch && (in.continuous || in.feature_path || in.records_only))
        p.refused = "wire records straight from the expansion: dense FramePerfect batches without feature mode only "
                    "(otherwise integrate events and serialise them with adder_hip_wire_events_device)";
    else if (in.records_only && (generic || in.continuous || in.feature_path))
        p.refused = "records can be handed out in the lean regime only (Collapse, delta_t_max <= time_spanned, no feature "
                    "mode, no generic batch before): gather events instead";
    return p;
}

// Where (frame slot, segment) parks its records (park_offset), once alloc_scratch has fixed the chunk and the bytes of
// one segment's slot.  Batches launched one frame at a time park frame-major, blocked ones in groups of the 16 segments
// an expansion wave reads of one frame (adder_lpx_kernel's pair_stride needs a pair of segments adjacent; measured
// against the rotated segment-major layout: profiles/r03_ctx_spread.txt); per-event-record batches append to logs and
// use none.  False: the ring does not fit a group layout (the segment count is padded to a multiple of 16 in
// adder_hip_create, and kMaxChunk slots of the largest kind take well below 2^32 bytes per group).
constexpr uint32_t kParkGroupShift = 4u;
inline bool batch_park_layout(uint32_t log_cap, uint32_t launch_depth, uint32_t num_waves, uint32_t chunk, uint32_t park_bytes,
                              ParkLayout *out) {
    const uint32_t pb = park_bytes;
    if (log_cap) {
        *out = ParkLayout{0u, 0u, 0u, 0u, 31u, 0xffffffffu};
    } else if (launch_depth == 1u && (uint64_t)num_waves * pb <= 0xffffffffull) {
        *out = ParkLayout{31u, 0u, num_waves * pb, pb, 31u, 0xffffffffu};
    } else {
        if ((num_waves & ((1u << kParkGroupShift) - 1u)) || ((uint64_t)chunk * pb << kParkGroupShift) > 0xffffffffull) return false;
        *out = ParkLayout{kParkGroupShift, (chunk * pb) << kParkGroupShift, pb << kParkGroupShift, pb, 31u, 0xffffffffu};
    }
    return true;
}

}  // namespace adder
