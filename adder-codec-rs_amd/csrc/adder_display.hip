// adder_display.hip -- Video::display_frame_features (video.rs:742-744, 1062-1088): the running plane with a white
// cross (draw_feature_coord, utils/viz.rs:94-120) on every feature (ShowFeatureMode::Hold) or on every feature the last
// frame found new (Instant).  Written as a GATHER: every output byte asks whether a member lies within the cross's reach
// of its pixel (adder_pixel.hpp display_under_cross), so the copy and the crosses need no ordering between them and
// overlapping crosses need no atomics.
//
// A workgroup takes kDisplayRows rows x kDisplayTileBytes bytes of the [rows][width][channels] plane, a wave per row.
// The members of the tile's pixels and of kCrossReach pixels around them go to LDS first (0 / 1 bytes; outside the plane:
// 0).  A lane then produces the 16 bytes of its row that share one 16-byte line of the DESTINATION (the first lane's
// line starts up to 15 bytes in front of the tile: a wave covers 63 * 16 bytes of the row whatever the alignment) and
// stores them as one dwordx4 when the line lies inside the row's part of the tile, byte by byte at its edges -- so any
// destination address and any row length are served, aligned ones with full-width stores.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "adder_kernels.h"

namespace adder {

constexpr uint32_t kDisplayRows = 4;                        // rows of a tile = waves of a workgroup
constexpr uint32_t kDisplayTileBytes = 63 * 16;             // bytes of a row one wave covers
constexpr uint32_t kDisplayWinW = kDisplayTileBytes + 2 * kCrossReach;  // pixels of a window row (one channel: most)
constexpr uint32_t kDisplayWinH = kDisplayRows + 2 * kCrossReach;

struct DisplayWindow {  // the tile's members in LDS: pixel (x, y) of the plane at win[(y - y0) * kDisplayWinW + (x - x0)]
    const uint8_t *win;
    int x0, y0;
    __device__ __forceinline__ bool operator()(uint32_t x, uint32_t y) const {
        return win[((int)y - y0) * (int)kDisplayWinW + ((int)x - x0)] != 0u;
    }
};

template <uint32_t CH>
__global__ __launch_bounds__(kDisplayRows * 64) void adder_display_kernel(const uint8_t *__restrict__ running,
                                                                         const uint8_t *__restrict__ member,
                                                                         const uint32_t *__restrict__ stamp,
                                                                         uint32_t stamp_val, uint32_t width, uint32_t rows,
                                                                         uint8_t *__restrict__ dst) {
    __shared__ uint8_t s_win[kDisplayWinH * kDisplayWinW];
    const uint32_t rowlen = width * CH;
    const uint32_t tile_b0 = blockIdx.x * kDisplayTileBytes;  // first byte of the tile inside a row (< rowlen)
    const uint32_t tile_y0 = blockIdx.y * kDisplayRows;
    const uint32_t tile_b1 = min(tile_b0 + kDisplayTileBytes, rowlen);  // one past the tile's last byte of a row
    // the window: the tile's pixels and kCrossReach around them, in plane coordinates (may start outside the plane)
    const int wx0 = (int)(tile_b0 / CH) - kCrossReach, wy0 = (int)tile_y0 - kCrossReach;
    const uint32_t win_w = (tile_b1 - 1u) / CH - tile_b0 / CH + 1u + 2u * kCrossReach;  // <= kDisplayWinW
    for (uint32_t i = threadIdx.x; i < kDisplayWinH * win_w; i += kDisplayRows * 64u) {
        const uint32_t wy = i / win_w, wx = i - wy * win_w;
        const int x = wx0 + (int)wx, y = wy0 + (int)wy;
        uint8_t m = 0u;
        if (x >= 0 && x < (int)width && y >= 0 && y < (int)rows) {
            const size_t p = (size_t)y * width + (size_t)x;
            m = stamp ? (stamp[p] == stamp_val ? 1u : 0u) : (member[p] != 0u ? 1u : 0u);
        }
        s_win[wy * kDisplayWinW + wx] = m;
    }
    __syncthreads();
    const uint32_t y = tile_y0 + threadIdx.x / 64u, lane = threadIdx.x & 63u;
    if (y >= rows) return;
    const DisplayWindow mw{s_win, wx0, wy0};
    const size_t row0 = (size_t)y * rowlen;
    const uint32_t mis = (uint32_t)((uintptr_t)(dst + row0 + tile_b0) & 15u);
    // the lane's line: bytes [lo, lo + 16) of the row; lo may lie in front of the tile for lane 0
    const int lo = (int)tile_b0 - (int)mis + (int)lane * 16;
    if (lo >= (int)tile_b1) return;
    uint32_t v[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int r = lo + k;
        if (r < (int)tile_b0 || r >= (int)tile_b1) continue;
        const uint32_t x = (uint32_t)r / CH, c = (uint32_t)r - x * CH;
        uint32_t byte = running[row0 + (uint32_t)r];
        if (display_drawn_channel(c, CH) && display_under_cross(mw, width, rows, x, y)) byte = 255u;
        v[k >> 2] |= byte << (8 * (k & 3));
    }
    if (lo >= (int)tile_b0 && lo + 16 <= (int)tile_b1) {
        *reinterpret_cast<uint4 *>(dst + row0 + (uint32_t)lo) = make_uint4(v[0], v[1], v[2], v[3]);  // 16-byte aligned
    } else {
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int r = lo + k;
            if (r >= (int)tile_b0 && r < (int)tile_b1) dst[row0 + (uint32_t)r] = (uint8_t)(v[k >> 2] >> (8 * (k & 3)));
        }
    }
}

}  // namespace adder

using namespace adder;

extern "C" hipError_t adder_launch_display(const uint8_t *running, const uint8_t *member, const uint32_t *stamp,
                                           uint32_t stamp_val, uint32_t width, uint32_t rows, uint32_t channels, uint8_t *dst,
                                           hipStream_t stream) {
    if (!running || !dst || (!member && !stamp) || !width || !rows || (channels != 1u && channels != 3u))
        return hipErrorInvalidValue;
    const uint32_t rowlen = width * channels;
    const dim3 grid((rowlen + kDisplayTileBytes - 1u) / kDisplayTileBytes, (rows + kDisplayRows - 1u) / kDisplayRows);
    if (channels == 1u)
        hipLaunchKernelGGL((adder_display_kernel<1u>), grid, dim3(kDisplayRows * 64u), 0, stream, running, member, stamp, stamp_val,
                           width, rows, dst);
    else
        hipLaunchKernelGGL((adder_display_kernel<3u>), grid, dim3(kDisplayRows * 64u), 0, stream, running, member, stamp, stamp_val,
                           width, rows, dst);
    return hipGetLastError();
}
