// adder_color_kernels.h -- between adder_color.hip and its callers: adder_color_api.cpp and the context's *_rgb entry
// points (include/adder_color.h and include/adder_hip.h are the public side).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace adder {

constexpr uint32_t kColorBlockX = 64;      // lanes along a row: one wave, four pixels per lane on the dword path
constexpr uint32_t kColorBlockY = 4;       // rows of a block
constexpr uint32_t kColorMaxBlocksX = 64;  // the grid is clamped in every dimension and strided beyond:
constexpr uint32_t kColorMaxBlocksY = 256; //   64 * 64 * 4 pixels along a row, 1024 rows, and
constexpr uint32_t kColorMaxBlocks = 16384;  // this many blocks in all (frames share what the plane leaves)

// Queues src [num_frames][rows][width][3] -> dst [num_frames][rows][width] on `stream`, strides in bytes (none of them
// 0 here).  The caller has checked the arguments: the kernel reads 3 * width and writes width bytes of every row and
// touches nothing else.
hipError_t color_to_gray_launch(const uint8_t *d_src, uint64_t src_row_stride, uint64_t src_frame_stride, uint8_t *d_dst,
                                uint64_t dst_row_stride, uint64_t dst_frame_stride, uint32_t width, uint32_t rows,
                                uint32_t num_frames, hipStream_t stream);

}  // namespace adder
