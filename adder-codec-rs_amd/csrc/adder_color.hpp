// adder_color.hpp -- one pixel of the reference's colour-to-gray step (utils/cv.rs:215-232, called by Framed::consume,
// framed.rs:127-134, whenever the source is colour and the transcode is not):
//
//     gray = (ch0 as f64 * 0.114 + ch1 as f64 * 0.587 + ch2 as f64 * 0.299) as u8
//
// Host and device.  The expression is f64, left to right, every product and every sum rounded on its own, then Rust's
// saturating `as u8`.  The byte depends on that: of the 2^24 triples, fusing both sums into FMAs changes 2 685, one FMA
// 1 488, the integer form (114 a + 587 b + 299 c) / 1000 changes 1 957 and f32 2 041.
//
// The library is built with -ffp-contract=off, but this function does not lean on the flag -- nor on a contraction
// pragma, which -ffp-contract=fast overrides (hipcc formed ten v_fma_f64 in the kernel under it).  Each product passes
// through an empty asm statement as an in/out register operand: the sums' operands are then values the compiler knows
// nothing about, so no multiply is left for it to fuse into an add, whatever the flags.  The statement emits no code.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ADDER_COLOR_HD __host__ __device__ __forceinline__
#else
#define ADDER_COLOR_HD inline
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define ADDER_COLOR_ROUNDED(v) asm("" : "+v"(v))  // a VGPR pair
#elif defined(__x86_64__) || defined(__i386__)
#define ADDER_COLOR_ROUNDED(v) asm("" : "+x"(v))  // an SSE register
#elif defined(__aarch64__)
#define ADDER_COLOR_ROUNDED(v) asm("" : "+w"(v))
#else
#define ADDER_COLOR_ROUNDED(v) asm("" : "+m"(v))
#endif

namespace adder {

ADDER_COLOR_HD uint8_t color_to_gray_px(uint8_t ch0, uint8_t ch1, uint8_t ch2) {
    double p0 = (double)ch0 * 0.114;
    double p1 = (double)ch1 * 0.587;
    double p2 = (double)ch2 * 0.299;
    ADDER_COLOR_ROUNDED(p0);
    ADDER_COLOR_ROUNDED(p1);
    ADDER_COLOR_ROUNDED(p2);
    const double v = (p0 + p1) + p2;
    // `as u8`: saturating, NaN -> 0 (neither can happen: 0 <= v <= 255.0, white gives exactly 255.0)
    return v >= 255.0 ? (uint8_t)255 : (v > 0.0 ? (uint8_t)(int32_t)v : (uint8_t)0);
}

}  // namespace adder
