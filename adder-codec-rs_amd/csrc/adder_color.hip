// adder_color.hip -- colour frames to gray (include/adder_color.h; utils/cv.rs:215-232 as Framed::consume calls it).
//
// [num_frames][rows][width][3] u8 -> [num_frames][rows][width] u8, byte strides on both sides.  Memory bound: 3 bytes
// in, 1 byte out per pixel; the arithmetic is color_to_gray_px (adder_color.hpp), five f64 operations per pixel.
//   * A block is 64 x 4 threads: a wave per row, its lanes side by side along the row.  Lane q owns pixels 4q .. 4q + 3.
//   * Dword path: the row's first source byte AND its first destination byte are 4-byte aligned, and all four pixels
//     lie inside the row.  Three aligned dword loads (source bytes 12q .. 12q + 11), one dword store (destination bytes
//     4q .. 4q + 3); a wave reads 768 and writes 256 contiguous bytes.
//   * Byte path: everything else -- the row's tail (width % 4 pixels) and rows that start off the 4-byte grid.  Byte
//     loads, byte stores, never past `width`.  The choice is per row (wave-uniform), so a packed clip of odd width runs
//     the dword path on the rows that happen to be aligned.
//   * One launch covers all frames: the grid is clamped in x (pixels), y (rows) and z (frames) and every dimension is
//     strided in 64-bit counters (adder_color_kernels.h).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "adder_color.hpp"
#include "adder_color_kernels.h"

namespace adder {

__global__ __launch_bounds__(kColorBlockX *kColorBlockY) void color_to_gray_kernel(
    const uint8_t *__restrict__ src, uint64_t src_row_stride, uint64_t src_frame_stride, uint8_t *__restrict__ dst,
    uint64_t dst_row_stride, uint64_t dst_frame_stride, uint32_t width, uint32_t rows, uint32_t num_frames) {
    const uint64_t quads = (uint64_t)(width >> 2) + ((width & 3u) != 0u ? 1u : 0u);  // lanes' worth of a row
    const uint64_t step_q = (uint64_t)gridDim.x * kColorBlockX, step_r = (uint64_t)gridDim.y * kColorBlockY;
    for (uint64_t f = blockIdx.z; f < num_frames; f += gridDim.z) {
        for (uint64_t r = (uint64_t)blockIdx.y * kColorBlockY + threadIdx.y; r < rows; r += step_r) {
            const uint8_t *s = src + f * src_frame_stride + r * src_row_stride;
            uint8_t *d = dst + f * dst_frame_stride + r * dst_row_stride;
            const bool aligned = (((uintptr_t)s | (uintptr_t)d) & 3u) == 0u;
            for (uint64_t q = (uint64_t)blockIdx.x * kColorBlockX + threadIdx.x; q < quads; q += step_q) {
                const uint64_t x0 = q * 4u;  // first pixel of this lane (< width)
                if (aligned && x0 + 4u <= width) {
                    const uint32_t *p = reinterpret_cast<const uint32_t *>(s + x0 * 3u);
                    const uint32_t w0 = p[0], w1 = p[1], w2 = p[2];
                    const uint32_t g0 = color_to_gray_px((uint8_t)w0, (uint8_t)(w0 >> 8), (uint8_t)(w0 >> 16));
                    const uint32_t g1 = color_to_gray_px((uint8_t)(w0 >> 24), (uint8_t)w1, (uint8_t)(w1 >> 8));
                    const uint32_t g2 = color_to_gray_px((uint8_t)(w1 >> 16), (uint8_t)(w1 >> 24), (uint8_t)w2);
                    const uint32_t g3 = color_to_gray_px((uint8_t)(w2 >> 8), (uint8_t)(w2 >> 16), (uint8_t)(w2 >> 24));
                    *reinterpret_cast<uint32_t *>(d + x0) = g0 | (g1 << 8) | (g2 << 16) | (g3 << 24);
                } else {
                    const uint32_t n = (uint32_t)((uint64_t)width - x0 < 4u ? (uint64_t)width - x0 : 4u);
                    for (uint32_t k = 0; k < n; ++k) {
                        const uint8_t *px = s + (x0 + k) * 3u;
                        d[x0 + k] = color_to_gray_px(px[0], px[1], px[2]);
                    }
                }
            }
        }
    }
}

// the launch's grid for [num_frames][rows][width] pixels: clamped per dimension, then the frames to what the plane leaves
static dim3 color_grid(uint32_t width, uint32_t rows, uint32_t num_frames) {
    const uint64_t quads = (uint64_t)(width >> 2) + ((width & 3u) != 0u ? 1u : 0u);
    const uint64_t bx = (quads + kColorBlockX - 1u) / kColorBlockX, by = ((uint64_t)rows + kColorBlockY - 1u) / kColorBlockY;
    const uint32_t gx = (uint32_t)(bx < 1u ? 1u : bx > kColorMaxBlocksX ? kColorMaxBlocksX : bx);
    const uint32_t gy = (uint32_t)(by < 1u ? 1u : by > kColorMaxBlocksY ? kColorMaxBlocksY : by);
    const uint32_t fz = kColorMaxBlocks / (gx * gy);  // >= 1: a plane's share is at most 64 * 256 blocks
    return dim3(gx, gy, num_frames < 1u ? 1u : (num_frames < fz ? num_frames : fz));
}

hipError_t color_to_gray_launch(const uint8_t *d_src, uint64_t src_row_stride, uint64_t src_frame_stride, uint8_t *d_dst,
                                uint64_t dst_row_stride, uint64_t dst_frame_stride, uint32_t width, uint32_t rows,
                                uint32_t num_frames, hipStream_t stream) {
    hipLaunchKernelGGL(color_to_gray_kernel, color_grid(width, rows, num_frames), dim3(kColorBlockX, kColorBlockY), 0, stream, d_src,
                       src_row_stride, src_frame_stride, d_dst, dst_row_stride, dst_frame_stride, width, rows, num_frames);
    return hipGetLastError();
}

}  // namespace adder
