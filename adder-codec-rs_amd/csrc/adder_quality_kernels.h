// adder_quality_kernels.h -- between adder_quality_api.cpp and adder_quality.hip (include/adder_quality.h is the public side).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace adder {

constexpr uint32_t kQualBlock = 256;                  // threads of every quality kernel
constexpr uint32_t kSsimTileW = kQualBlock - 8;       // windows per tile row: their 248 + 7 pixel columns fit one block
constexpr uint32_t kSsimTileH = 32;                   // window rows per tile
constexpr uint32_t kSseBytesPerBlock = kQualBlock * 16u * 8u;  // SSE: eight 16-byte loads per lane
constexpr uint32_t kSseMaxBlocks = 1024;              // SSE blocks per frame at most

// C1 = (K1 * L)^2, C2 = (K2 * L)^2 (cv.rs:367-372), each evaluated in f64
constexpr double kSsimC1 = (0.01 * 255.0) * (0.01 * 255.0);
constexpr double kSsimC2 = (0.03 * 255.0) * (0.03 * 255.0);

struct QualityFrameSums {      // per frame, written by the second stage
    unsigned long long sse;    // sum of (a - b)^2 over every element
    double ssim64[3];          // per channel: sum of 64 * r over its windows, in the library's fixed order
};

struct QualityShape {          // depends on the plane alone: a frame's partials do not depend on the call
    uint32_t width, height, channels;
    uint32_t tiles_x, tiles_y; // SSIM tiles of a plane (0 x 0 when it has no 8x8 window)
    uint32_t sse_blocks;       // SSE blocks per frame
    uint64_t frame_bytes;      // width * height * channels
    uint64_t windows;          // (height - 7) * (width - 7), 0 when the plane has none
};

QualityShape quality_shape(uint32_t width, uint32_t height, uint32_t channels);
// Frames per launch group: keeps every grid within 65535 rows and 2^32 work-items.
uint32_t quality_group_frames(const QualityShape &s);
// Queues the metrics of n frame pairs on `stream`: SSE partials, then (ssim) the SSIM tiles -- writing the per-window
// map when d_map is not null -- and the fixed-order combine into d_sums[0 .. n).  Scratch: sse_part n * sse_blocks,
// ssim_part n * channels * tiles_x * tiles_y (ssim only).
hipError_t quality_run(const QualityShape &s, const uint8_t *d_a, const uint8_t *d_b, uint32_t n, bool ssim,
                       double *d_map, unsigned long long *sse_part, double *ssim_part, QualityFrameSums *d_sums,
                       hipStream_t stream);

}  // namespace adder
