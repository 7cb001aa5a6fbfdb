// adder_variant.hpp -- the variant word: which frame kernel and which expansion a batch runs (adder_launch_frame,
// adder_launch_expand), the decisions the host derives from it, and the scratch ring's layout.  No HIP: the batch
// plan's CPU test includes it too.
#pragma once
#include <stdint.h>

#include "../../include/adder_hip.h"

namespace adder {

// Bits of the variant word.  Their values are part of the graph cache key (get_graph) and of the per-frame ring's
// hand-over key (frame_submit_impl): they do not move.
constexpr uint32_t kVarCollapse = 1u;       // MultiMode::Collapse
constexpr uint32_t kVarAbsT = 2u;           // TimeMode::AbsoluteT
constexpr uint32_t kVarGeneric = 4u;        // the generic step (any arena depth)
constexpr uint32_t kVarContinuous = 8u;     // Mode::Continuous
constexpr uint32_t kVarWide = 16u;          // the band has >= 4 units: the 4-units-per-lane one-frame kernel may run
constexpr uint32_t kVarBounded = 32u;       // the bounded Collapse step (with generic: its per-event record format)
constexpr uint32_t kVarLeanLog = 64u;       // lean records in per-segment logs (batches that hand their records out)
constexpr uint32_t kVarConstRuns = 128u;    // constant runs (adder_cr_kernel)
constexpr uint32_t kVarLeanRuns = 256u;     // lean runs (adder_lr_kernel)
constexpr uint32_t kVarRunRecords = 512u;   // run records (adder_rr_kernel)
constexpr uint32_t kVarWire = 1024u;        // the expansion writes the raw sink's records instead of AdderEvents
constexpr uint32_t kVarLazyState = 2048u;   // more launches of this batch follow (variant_lazy_state_bit)
constexpr uint32_t kVarPacked = 4096u;      // lean runs in packed bytes (adder_lp_kernel / adder_lpx_kernel)
constexpr uint32_t kVarPackedRgb = 8192u;   // ... on a three-channel plane (11-byte wire records)
constexpr uint32_t kVarView = 16384u;       // the side plane shows D, DeltaT or SAE: the kernels' view instantiations
constexpr uint32_t kVarKeepUndo = 32768u;   // this launch keeps the batch's two-plane undo copy (variant_keep_undo_bit)
constexpr uint32_t kVarKeyMask = 0xffffu;   // the bits the graph cache key holds

// The frame kernel a variant runs (ADDER_KERNEL_*), in adder_launch_frame's order of precedence.
inline unsigned variant_frame_kernel(uint32_t v) {
    if (v & kVarContinuous) return ADDER_KERNEL_CONTINUOUS;
    if (v & kVarRunRecords) return ADDER_KERNEL_RUN_RECORDS;
    if (v & kVarConstRuns) return ADDER_KERNEL_CONSTANT_RUNS;
    if (v & kVarBounded) return ADDER_KERNEL_BOUNDED;
    if (v & kVarGeneric) return ADDER_KERNEL_GENERIC;
    if (v & kVarPacked) return ADDER_KERNEL_LEAN_RUNS_PACKED;
    if (v & kVarLeanRuns) return ADDER_KERNEL_LEAN_RUNS;
    return ADDER_KERNEL_LEAN;
}

// The frame kernels that zero the frame-offset entries themselves (chain_zero), so that the scan's blocks can chain
// the offsets (adder_scan_kernel CHAIN): the integer-state kernels and the bounded Collapse kernel.
inline bool variant_scan_chains(uint32_t v) {
    const unsigned k = variant_frame_kernel(v);
    return k != ADDER_KERNEL_CONTINUOUS && k != ADDER_KERNEL_GENERIC && k != ADDER_KERNEL_LEAN;
}

// The integer-state kernels (lean runs, run records) keep their whole state in the header, delta_t and last_fired_t
// planes; the other level-0 planes and the levels are derived from it (divisions, and for run records a store per level).
// A launch that is followed by another launch of the same batch leaves them stale: only the batch's last launch brings
// the planes to the resident form every other kernel, a rollback or the next batch reads.  (Run records: 30 us of a
// 160 us launch were this epilogue.)
inline uint32_t variant_lazy_state_bit(uint32_t v, bool more_launches, bool running_enabled) {
    return (more_launches && (v & (kVarLeanRuns | kVarRunRecords)) && !running_enabled) ? kVarLazyState : 0u;
}

// The packed lean-runs kernel loads a unit's whole state -- header and delta_t (lr_unpack) -- before its first frame and
// writes no state plane until its last: the FIRST launch of a batch that keeps the two-plane undo copy stores what it
// loaded into the copy's planes (BatchArgs::snap_hdr / snap_dt), and the host queues no copy in front of the batch.
inline uint32_t variant_keep_undo_bit(uint32_t v, bool first_launch, bool two_plane_undo) {
    return (first_launch && two_plane_undo && (v & kVarPacked)) ? kVarKeepUndo : 0u;
}

// Graph instances a batch length tries before it settles (get_graph): a batch of a single chunk has no second branch
// to overlap, and per-event-record batches are captured on one stream -- one candidate is all they need.
inline uint32_t variant_graph_candidates(uint32_t v, uint32_t num_frames, uint32_t chunk, uint32_t candidates) {
    return (num_frames > chunk && !(v & kVarGeneric) && candidates > 1u) ? candidates : 1u;
}

// Where a batch parks its records inside a chunk of the scratch ring (adder_kernels.h park_offset; batch_park_layout).
struct ParkLayout {
    uint32_t group_shift;   // log2 of the segments per group (31: one group = frame-major)
    uint32_t group_stride;  // bytes between consecutive groups
    uint32_t frame_stride;  // bytes between consecutive frame slots of one segment
    uint32_t seg_stride;    // bytes between consecutive segments inside a group
    // Rotation of the frame slots: segment s keeps frame slot fi at (fi + (s >> rot_shift)) & rot_mask.  The kernels
    // honour it; the host's layouts leave it off (rot_shift = 31, rot_mask = 0xffffffff).
    uint32_t rot_shift, rot_mask;
};

}  // namespace adder
