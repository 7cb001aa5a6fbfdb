// adder_color_api.cpp -- C-ABI of the colour-to-gray step (include/adder_color.h): the argument checks both forms share,
// the launch of adder_color.hip, and the CPU loop over the same per-pixel function (adder_color.hpp).
#include <hip/hip_runtime.h>

#include "../../include/adder_color.h"
#include "adder_api_util.hpp"
#include "adder_color.hpp"
#include "adder_color_kernels.h"

using namespace adder;

static thread_local std::string g_color_error;

static int cfail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    api_fail(g_color_error, code, fmt, ap);
    va_end(ap);
    return code;
}

namespace {

struct ColorStrides {
    size_t src_row, src_frame, dst_row, dst_frame;
};

// bytes from a side's first to behind its last byte: (frames - 1) * frame + (rows - 1) * row + row_bytes; false: no size_t
bool span_bytes(size_t row_bytes, size_t row_stride, size_t frame_stride, uint32_t rows, uint32_t frames, size_t *out) {
    size_t a = 0, b = 0;
    if (__builtin_mul_overflow((size_t)(frames - 1u), frame_stride, &a)) return false;
    if (__builtin_mul_overflow((size_t)(rows - 1u), row_stride, &b)) return false;
    if (__builtin_add_overflow(a, b, &a)) return false;
    return !__builtin_add_overflow(a, row_bytes, out);
}

// one side's strides with the zeros filled in; false: shorter than what they step over
bool fill_strides(size_t row_bytes, uint32_t rows, size_t *row_stride, size_t *frame_stride) {
    if (*row_stride == 0) *row_stride = row_bytes;
    if (*row_stride < row_bytes) return false;
    size_t frame_span = 0;
    if (!span_bytes(row_bytes, *row_stride, 0, rows, 1u, &frame_span)) return false;
    if (*frame_stride == 0 && __builtin_mul_overflow(*row_stride, (size_t)rows, frame_stride)) return false;
    return *frame_stride >= frame_span;
}

int check_call(const uint8_t *src, uint8_t *dst, uint32_t width, uint32_t rows, uint32_t num_frames, ColorStrides *st) {
    if (!src || !dst) return cfail(ADDER_E_BAD_PARAMS, "null pointer");
    if (width == 0 || rows == 0 || num_frames == 0)
        return cfail(ADDER_E_BAD_PARAMS, "zero extent (%u frames of %u x %u)", num_frames, width, rows);
    const size_t src_row_bytes = (size_t)width * 3u, dst_row_bytes = width;
    if (!fill_strides(src_row_bytes, rows, &st->src_row, &st->src_frame))
        return cfail(ADDER_E_BAD_PARAMS, "source strides (row %zu, frame %zu) are smaller than a row of %zu bytes / a frame of %u rows",
                     st->src_row, st->src_frame, src_row_bytes, rows);
    if (!fill_strides(dst_row_bytes, rows, &st->dst_row, &st->dst_frame))
        return cfail(ADDER_E_BAD_PARAMS, "destination strides (row %zu, frame %zu) are smaller than a row of %zu bytes / a frame of %u rows",
                     st->dst_row, st->dst_frame, dst_row_bytes, rows);
    size_t src_span = 0, dst_span = 0;
    const uintptr_t s = (uintptr_t)src, d = (uintptr_t)dst;
    uintptr_t s_end = 0, d_end = 0;
    if (!span_bytes(src_row_bytes, st->src_row, st->src_frame, rows, num_frames, &src_span) ||
        !span_bytes(dst_row_bytes, st->dst_row, st->dst_frame, rows, num_frames, &dst_span) ||
        __builtin_add_overflow(s, (uintptr_t)src_span, &s_end) || __builtin_add_overflow(d, (uintptr_t)dst_span, &d_end))
        return cfail(ADDER_E_BAD_PARAMS, "the frames' byte range does not fit the address space");
    if (s < d_end && d < s_end) return cfail(ADDER_E_BAD_PARAMS, "source and destination overlap");
    return ADDER_OK;
}

}  // namespace

extern "C" const char *adder_color_last_error(void) { return g_color_error.c_str(); }

extern "C" int adder_color_to_gray_device(const uint8_t *d_src, size_t src_row_stride, size_t src_frame_stride, uint8_t *d_dst,
                                          size_t dst_row_stride, size_t dst_frame_stride, uint32_t width, uint32_t rows,
                                          uint32_t num_frames, void *stream) {
    ColorStrides st{src_row_stride, src_frame_stride, dst_row_stride, dst_frame_stride};
    const int rc = check_call(d_src, d_dst, width, rows, num_frames, &st);
    if (rc != ADDER_OK) return rc;
    const hipError_t e = color_to_gray_launch(d_src, st.src_row, st.src_frame, d_dst, st.dst_row, st.dst_frame, width, rows,
                                              num_frames, (hipStream_t)stream);
    if (e != hipSuccess) return cfail(ADDER_E_HIP, "colour-to-gray launch failed: %s", hipGetErrorString(e));
    return ADDER_OK;
}

extern "C" int adder_color_to_gray_host(const uint8_t *src, size_t src_row_stride, size_t src_frame_stride, uint8_t *dst,
                                        size_t dst_row_stride, size_t dst_frame_stride, uint32_t width, uint32_t rows,
                                        uint32_t num_frames) {
    ColorStrides st{src_row_stride, src_frame_stride, dst_row_stride, dst_frame_stride};
    const int rc = check_call(src, dst, width, rows, num_frames, &st);
    if (rc != ADDER_OK) return rc;
    for (uint32_t f = 0; f < num_frames; ++f)
        for (uint32_t r = 0; r < rows; ++r) {
            const uint8_t *s = src + (size_t)f * st.src_frame + (size_t)r * st.src_row;
            uint8_t *d = dst + (size_t)f * st.dst_frame + (size_t)r * st.dst_row;
            for (size_t x = 0; x < width; ++x) d[x] = color_to_gray_px(s[3 * x], s[3 * x + 1], s[3 * x + 2]);
        }
    return ADDER_OK;
}
