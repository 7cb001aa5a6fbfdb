// adder_davis_logic.hpp -- the per-pixel arithmetic of the DAVIS chain (include/adder_davis.h; davis.rs:233-598 and
// :775-864), shared by the kernels of adder_davis.hip and the CPU forms of adder_davis_api.cpp (adder_davis_steps_host,
// _gaps_host, _frame_host).  Every cast stands where the C++ mirror's Davis has it; exp and log1p are the library's
// bit-exact binary64 routines, and the file is built with -ffp-contract=off like the rest of the library.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/adder_davis.h"
#include "adder_exp.hpp"
#include "adder_log1p.hpp"

namespace adder {

struct DavisConsts {  // what one call fixes
    float tpm;        // ticks per microsecond: (f32)tps / 1e6f
    float ref_f;      // (f32)ref_time
    double ref_d;     // (f64)ref_time
    double exp_on;    // exp(c)
    double exp_off;   // exp(-c)
    double ln_one;    // ln_1p(1.0), the high clamp (ln_1p(0.0) is 0.0)
};

__host__ __device__ inline DavisConsts davis_consts(double c, uint32_t tps, uint32_t ref_time) {
    DavisConsts k;
    k.tpm = (float)tps / 1e6f;
    k.ref_f = (float)ref_time;
    k.ref_d = (double)ref_time;
    k.exp_on = adder_exp(c);
    k.exp_off = adder_exp(-c);
    k.ln_one = dvs_log1p(1.0);
    return k;
}

// Rust's `as u8`: saturating, NaN -> 0
__host__ __device__ inline uint8_t davis_as_u8(double v) { return !(v > 0.0) ? 0u : (v >= 255.0 ? 255u : (uint8_t)v); }

// std::max(a, 0) as the mirror writes it: a NaN stays
__host__ __device__ inline float davis_max0(float a) { return a < 0.0f ? 0.0f : a; }
__host__ __device__ inline double davis_max0(double a) { return a < 0.0 ? 0.0 : a; }

// wrapping i64 difference (what a release build of the reference computes)
__host__ __device__ inline int64_t davis_delta(int64_t a, int64_t b) { return (int64_t)((uint64_t)a - (uint64_t)b); }

// utils/cv.rs:432-440; true when the value was clamped (and last ln rewritten)
__host__ __device__ inline bool davis_clamp_u8(double &val, double &ln, const DavisConsts &k) {
    if (val <= 0.0) {
        val = 0.0;
        ln = 0.0;
        return true;
    }
    if (val > 255.0) {
        val = 255.0;
        ln = k.ln_one;
        return true;
    }
    return false;
}

__host__ __device__ inline double davis_val(double ln) { return (adder_exp(ln) - 1.0) * 255.0; }

// check_dvs_before, and the second check of the previous packet's `after` events (davis.rs:287-294)
__host__ __device__ inline bool davis_event_passes(int64_t t, int64_t check1, int32_t check2_mode, int64_t check2) {
    if (!(t < check1)) return false;
    if (check2_mode == 1) return t > check2;
    if (check2_mode == 2) return t < check2;
    return true;
}

__host__ __device__ inline AdderSparseStep davis_step(uint32_t x, uint32_t y, uint8_t frame_val, uint16_t flags,
                                                      float intensity, float time) {
    AdderSparseStep s;
    s.x = (uint16_t)x;
    s.y = (uint16_t)y;
    s.c = ADDER_C_NONE;
    s.frame_val = frame_val;
    s.pad = flags;
    s.intensity = intensity;
    s.time = time;
    return s;
}

// A pixel's camera state while a lane (or the host loop) walks its events.  `val` caches (exp(ln) - 1) * 255 of the
// current ln: the value an unclamped event leaves is the next event's last_val, the same routine on the same bits.
struct DavisPixel {
    int64_t ts;
    double ln;
    double val;
    bool have_val;
};

__host__ __device__ inline DavisPixel davis_pixel(int64_t ts, double ln) { return DavisPixel{ts, ln, 0.0, false}; }

// One event that passed the checks (davis.rs:296-395): 0 or 2 steps into out[0..2)
__host__ __device__ inline uint32_t davis_event_steps(DavisPixel &px, uint32_t x, uint32_t y, int64_t t, bool on,
                                                      const DavisConsts &k, AdderSparseStep *out) {
    const int64_t dmicro = davis_delta(t, px.ts);
    if (dmicro == t) return 0u;  // the pixel has seen no frame yet
    const float dticks = (float)dmicro * k.tpm;
    if (dticks < 0.0f) return 0u;
    if (!px.have_val) px.val = davis_val(px.ln);
    const float first = davis_max0((float)px.val / k.ref_f * dticks);
    out[0] = davis_step(x, y, 0u, ADDER_SPARSE_NO_SIDE | ADDER_SPARSE_INTEGRATE_ONLY, first, dticks);
    px.ln *= on ? k.exp_on : k.exp_off;
    double v = davis_val(px.ln);
    px.have_val = !davis_clamp_u8(v, px.ln, k);
    px.val = v;
    out[1] = davis_step(x, y, davis_as_u8(v), ADDER_SPARSE_NO_SIDE | ADDER_SPARSE_TEST_ONLY, (float)v, 0.0f);
    px.ts = t;
    return 2u;
}

// integrate_frame_gaps for one pixel (davis.rs:468-598): the clamp rewrites ln even when the pixel is then skipped
__host__ __device__ inline uint32_t davis_gap_step(int64_t ts, double &ln, uint32_t x, uint32_t y, int64_t start,
                                                   const DavisConsts &k, AdderSparseStep *out) {
    double v = davis_val(ln);
    davis_clamp_u8(v, ln, k);
    const int64_t dmicro = davis_delta(start, ts);
    if (dmicro == start) return 0u;
    const float dticks = (float)dmicro * k.tpm;
    if (dticks <= 0.0f) return 0u;
    const double integration = davis_max0((v / k.ref_d) * (double)dticks);
    out[0] = davis_step(x, y, davis_as_u8(v), 0u, (float)integration, dticks);
    return 1u;
}

// what a push refuses in a frame it reads: ln_1p is undefined there
__host__ __device__ inline bool davis_frame_value_ok(double v) { return v > -1.0; }

// convert_to(CV_8U, 255.0): saturate_cast<uchar>(cvRound(v * 255)), round half to even
__host__ __device__ inline uint8_t davis_frame_u8(double v) {
    const double r = rint(v * 255.0);
    return (uint8_t)(r <= 0.0 ? 0.0 : (r >= 255.0 ? 255.0 : r));
}

// the frame's integration time (davis.rs:775-838)
__host__ __device__ inline float davis_frame_span(int32_t mode, int64_t start, int64_t end, uint32_t ref_time) {
    if (mode == ADDER_DAVIS_RAW_DAVIS) return (float)davis_delta(end, start);
    if (mode == ADDER_DAVIS_RAW_DVS) return 0.0f;
    return (float)ref_time;
}

// steps 5 and 6 for one pixel: its byte of image_8u and its new last ln
__host__ __device__ inline uint8_t davis_frame_pixel(int32_t mode, double frame, double &ln) {
    if (mode == ADDER_DAVIS_RAW_DVS) {
        ln = dvs_log1p(0.5);
        return 0u;
    }
    ln = dvs_log1p(frame);
    return davis_frame_u8(frame);
}

}  // namespace adder
