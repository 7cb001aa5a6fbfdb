// adder_fast_kernels.h -- between adder_fast_api.cpp and adder_fast.hip (include/adder_fast.h is the public side).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace adder {

constexpr uint32_t kFastBlock = 256;   // threads of every kernel here
constexpr uint32_t kFastTileW = 128;   // pixels of a score tile: 32 lanes of 4 adjacent pixels ...
constexpr uint32_t kFastTileH = 32;    // ... by 8 rows, four times
constexpr uint32_t kFastHaloX = 4;     // staged columns each side: the ring's 3, rounded up to a dword of LDS
constexpr uint32_t kFastHaloY = 3;
constexpr uint32_t kFastCountBlocks = 64;  // blocks per frame of the counting kernel at most

struct FastFrameSums {         // per frame: integer counters, the same in any order
    unsigned long long gt;     // kept pixels
    unsigned long long pred;   // predicted positions (0 without a prediction)
    unsigned long long both;
};

struct FastShape {
    uint32_t width, height, channels;
    uint32_t tiles_x, tiles_y;
    uint64_t plane;            // width * height
    uint64_t frame_bytes;      // plane * channels
};

FastShape fast_shape(uint32_t width, uint32_t height, uint32_t channels);
// Frames per launch group: every grid and every scan stays below 2^31 work-items and 65536 rows.
uint32_t fast_group_frames(const FastShape &s);
// Temporary storage the flag scan of one group takes.
size_t fast_scan_temp_bytes(const FastShape &s, uint32_t n);

// Queues the detector over n frames: the score tiles, then (nonmax) the 3x3 suppression.  d_mask [n][H][W] is always
// written; d_score [n][H][W] is needed with nonmax and otherwise written when not null.
hipError_t fast_detect_run(const FastShape &s, const uint8_t *d_frames, uint32_t n, int threshold, bool nonmax,
                           uint8_t *d_mask, uint8_t *d_score, hipStream_t stream);
// Zeroes d_sums[0 .. n) and queues the counting of d_mask (0 / 1) against d_pred (nonzero = predicted; may be null).
hipError_t fast_count_run(const FastShape &s, const uint8_t *d_mask, const uint8_t *d_pred, uint32_t n,
                          FastFrameSums *d_sums, hipStream_t stream);
// Queues the compaction of d_mask's set pixels to d_xy (x | y << 16, raster order, frame after frame).  counts[n]: the
// frames' totals (the host has them from fast_count_run); offs: n-in-a-group * plane words; cap: the room of d_xy.
hipError_t fast_compact_run(const FastShape &s, const uint8_t *d_mask, uint32_t n, const uint64_t *counts,
                            uint32_t *offs, void *temp, size_t temp_bytes, uint32_t *d_xy, uint64_t cap,
                            hipStream_t stream);
// *d_bad |= 1 if one of the n coordinates lies outside the plane (the caller zeroes it)
hipError_t fast_xy_check_run(const FastShape &s, const uint32_t *d_xy, uint64_t n, uint32_t *d_bad, hipStream_t stream);
// clears d_mask [H][W] and sets 1 at each coordinate (those outside the plane are skipped)
hipError_t fast_xy_mask_run(const FastShape &s, const uint32_t *d_xy, uint64_t n, uint8_t *d_mask, hipStream_t stream);

}  // namespace adder
