/* adder_color.h -- C-ABI of the colour-to-gray step of a one-channel transcode (libadder_hip.so).
 *
 * The reference's decoder always delivers three-channel 8-bit frames; with color_input == false (adder_simulproc's
 * default) Framed::consume (transcoder/source/framed.rs:127-134) runs each of them through handle_color
 * (utils/cv.rs:215-232) before integrate_matrix:
 *
 *     gray = (ch0 as f64 * 0.114 + ch1 as f64 * 0.587 + ch2 as f64 * 0.299) as u8
 *
 * in f64, left to right, nothing fused, with Rust's saturating `as u8`.  Both functions below give that byte for every
 * one of the 2^24 triples (a gray pixel one off gives different events); the integer form (114 a + 587 b + 299 c) / 1000,
 * f32, or an FMA anywhere in the expression do not.
 *
 * src is [num_frames][rows][width][3] u8, dst is [num_frames][rows][width] u8.  Strides are in bytes; 0 means packed
 * (row: 3 * width resp. width; frame: rows * row stride).  Exactly `width` bytes of every destination row are written:
 * no stride padding, nothing in front of or behind the buffer.
 *
 * ADDER_E_BAD_PARAMS, before anything is done: a null pointer; width, rows or num_frames of 0; a row stride smaller
 * than a row, a frame stride smaller than the frame's rows span; byte ranges of src and dst that overlap (or whose
 * size does not fit a size_t).
 *
 * The context-bound forms -- colour frames straight into a channels == 1 context -- are adder_hip_integrate_rgb_device,
 * adder_hip_integrate_wire_rgb_device, adder_hip_integrate_batch_rgb and adder_hip_frame_submit_rgb (adder_hip.h). */
#ifndef ADDER_COLOR_H
#define ADDER_COLOR_H

#include <stddef.h>
#include <stdint.h>

#include "adder_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Device pointers (of the current device).  One kernel launch for all frames, asynchronous on `stream` (NULL: the
 * default stream), ordered like any other work queued there.  A row whose first source byte and first destination
 * byte are both 4-byte aligned moves as dwords; other rows, and the last width % 4 pixels of every row, as bytes.
 * ADDER_E_HIP when the launch fails. */
int adder_color_to_gray_device(const uint8_t *d_src, size_t src_row_stride, size_t src_frame_stride, uint8_t *d_dst,
                               size_t dst_row_stride, size_t dst_frame_stride, uint32_t width, uint32_t rows,
                               uint32_t num_frames, void *stream);
/* The same on the CPU for host pointers: touches no device (it runs without one). */
int adder_color_to_gray_host(const uint8_t *src, size_t src_row_stride, size_t src_frame_stride, uint8_t *dst,
                             size_t dst_row_stride, size_t dst_frame_stride, uint32_t width, uint32_t rows,
                             uint32_t num_frames);
/* Describes the calling thread's last failure of the two functions above. */
const char *adder_color_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* ADDER_COLOR_H */
