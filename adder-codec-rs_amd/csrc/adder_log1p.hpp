// adder_log1p.hpp -- binary64 log1p, host and device, equal bit for bit to the platform libm's (glibc 2.35, whose
// scalar log1p is Sun fdlibm's s_log1p.c with the polynomial regrouped into four partial products).  The reference's
// f64::ln_1p calls that libm function; OCML's device log1p is a different routine and may differ in the last bit,
// which can flip a DVS firing decision.  Built with -ffp-contract=off: no operation may be fused.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace adder {

__host__ __device__ inline int32_t l1p_hi(double x) { return (int32_t)(__builtin_bit_cast(uint64_t, x) >> 32); }
__host__ __device__ inline double l1p_with_hi(double x, int32_t h) {
    const uint64_t b = (__builtin_bit_cast(uint64_t, x) & 0xffffffffull) | ((uint64_t)(uint32_t)h << 32);
    return __builtin_bit_cast(double, b);
}

__host__ __device__ inline double dvs_log1p(double x) {
    const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10;
    const double Lp1 = 6.666666666666735130e-01, Lp2 = 3.999999999940941908e-01, Lp3 = 2.857142874366239149e-01,
                 Lp4 = 2.222219843214978396e-01, Lp5 = 1.818357216161805012e-01, Lp6 = 1.531383769920937332e-01,
                 Lp7 = 1.479819860511658591e-01;
    double hfsq, f = 0.0, c = 0.0, s, z, R, u;
    int32_t k = 1, hu = 0;
    const int32_t hx = l1p_hi(x), ax = hx & 0x7fffffff;
    if (hx < 0x3FDA827A) {  // x < 0.41422
        if (ax >= 0x3ff00000) {  // x <= -1.0
            if (x == -1.0) return -__builtin_inf();
            return (x - x) / (x - x);
        }
        if (ax < 0x3e200000) {  // |x| < 2^-29
            if (ax < 0x3c900000) return x;
            return x - x * x * 0.5;
        }
        if (hx > 0 || hx <= (int32_t)0xbfd2bec3) {  // -0.2929 < x < 0.41422
            k = 0;
            f = x;
            hu = 1;
        }
    }
    if (hx >= 0x7ff00000) return x + x;
    if (k != 0) {
        if (hx < 0x43400000) {
            u = 1.0 + x;
            hu = l1p_hi(u);
            k = (hu >> 20) - 1023;
            c = (k > 0) ? 1.0 - (u - x) : x - (u - 1.0);  // correction term
            c /= u;
        } else {
            u = x;
            hu = l1p_hi(u);
            k = (hu >> 20) - 1023;
            c = 0.0;
        }
        hu &= 0x000fffff;
        if (hu < 0x6a09e) {
            u = l1p_with_hi(u, hu | 0x3ff00000);  // normalise u
        } else {
            k += 1;
            u = l1p_with_hi(u, hu | 0x3fe00000);  // normalise u / 2
            hu = (0x00100000 - hu) >> 2;
        }
        f = u - 1.0;
    }
    hfsq = 0.5 * f * f;
    if (hu == 0) {  // |f| < 2^-20
        if (f == 0.0) {
            if (k == 0) return 0.0;
            c += k * ln2_lo;
            return k * ln2_hi + c;
        }
        R = hfsq * (1.0 - 0.66666666666666666 * f);
        if (k == 0) return f - R;
        return k * ln2_hi - ((R - (k * ln2_lo + c)) - f);
    }
    s = f / (2.0 + f);
    z = s * s;
    const double R1 = z * Lp1, z2 = z * z, R2 = Lp2 + z * Lp3, z4 = z2 * z2, R3 = Lp4 + z * Lp5, z6 = z4 * z2,
                 R4 = Lp6 + z * Lp7;
    R = R1 + z2 * R2 + z4 * R3 + z6 * R4;
    if (k == 0) return f - (hfsq - s * (hfsq + R));
    return k * ln2_hi - ((hfsq - (s * (hfsq + R) + (k * ln2_lo + c))) - f);
}

// event_to_frame_intensity (adder-to-dvs main.rs:450-460) for d <= 128, in the reference's order of operations
__host__ __device__ inline double dvs_intensity_ln(uint32_t d, uint32_t t, double ref) {
    if (d == 128u) return 0.0;
    const double p = __builtin_bit_cast(double, (uint64_t)(1023u + d) << 52);  // 2^d, exact
    if (t == 0u) return dvs_log1p((p * ref) / 255.0);
    return dvs_log1p(((p / (double)t) * ref) / 255.0);
}

}  // namespace adder
