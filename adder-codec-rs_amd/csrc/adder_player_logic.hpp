// adder_player_logic.hpp -- the arithmetic of the latest-event player (include/adder_player.h) that host and device
// share: the frame length, the event's display value, and the display schedule as a prefix minimum.
//
// The schedule.  The reference (adder_video_player.rs:122-131) makes one check per record position i, in stream order:
//     F_{i+1} = F_i + [cur_i > F_i * FL]          F = frame_count (F_0 carried, 1 at the start), cur_i = current_t
// cur never decreases.  Let T_i be the smallest F that stops the display at position i:
//     T_i = 0 when cur_i == 0;  unbounded when FL == 0 and cur_i > 0;  ceil(cur_i / FL) otherwise
// (F * FL < cur  <=>  F < cur / FL  <=>  F < ceil(cur / FL) for integers), so F_{i+1} = F_i + [F_i < T_i]
// = min(F_i + 1, max(F_i, T_i)).  With M_j = max(T_j, F_0), which never decreases either,
//     F_{i+1} = min(F_0 + i + 1,  min_{j <= i} (M_j + i - j)).
// Proof by induction.  Call the right side G_{i+1}, G_0 = F_0.  Taking j = i out of the minimum,
// G_{i+1} = min(G_i + 1, M_i); G_1 = min(F_0 + 1, M_0) is the serial step.  For i >= 1: G_i <= M_{i-1} <= M_i (the
// j = i - 1 term of G_i) and G_i >= F_0.  If T_i >= G_i then M_i = T_i = max(G_i, T_i).  If T_i < G_i then
// M_i >= G_i > T_i forces M_i = F_0 = G_i, and both sides give G_i.  So one inclusive prefix minimum of
// term_j = M_j - j gives every F_i, and the display marks are [F_i < T_i].
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ADDER_PLAYER_HD __host__ __device__ __forceinline__
#else
#define ADDER_PLAYER_HD inline
#endif

namespace adder {

constexpr uint64_t kPlayerUnbounded = 1ull << 62;  // above every frame count a stream can reach

// (tps as f64 / playback_fps) as u128, clamped to 2^32: current_t < 2^32 and F >= 1, so every FL >= 2^32 stops every
// display.  fps is finite and positive (checked at create); the quotient may still be +inf.
ADDER_PLAYER_HD uint64_t player_frame_length(uint32_t tps, double fps) {
    const double q = (double)tps / fps;
    return q >= 4294967296.0 ? (1ull << 32) : (uint64_t)q;
}

ADDER_PLAYER_HD uint64_t player_stop(uint32_t cur, uint64_t fl) {
    if (cur == 0u) return 0u;
    if (fl == 0u) return kPlayerUnbounded;
    return ((uint64_t)cur + fl - 1u) / fl;
}

// term_i = max(T_i, F_0) - i; its inclusive prefix minimum is `pmin`
ADDER_PLAYER_HD int64_t player_term(uint64_t stop, uint64_t f0, uint64_t i) {
    return (int64_t)(stop > f0 ? stop : f0) - (int64_t)i;
}

// F_i from pmin_{i-1} (unused at i == 0)
ADDER_PLAYER_HD uint64_t player_frame_count(uint64_t f0, uint64_t i, int64_t pmin_before) {
    if (i == 0u) return f0;
    const uint64_t a = f0 + i;
    const uint64_t b = (uint64_t)((int64_t)(i - 1u) + pmin_before);
    return a < b ? a : b;
}

ADDER_PLAYER_HD uint32_t player_round_up(uint32_t t, uint32_t ref) {  // u32, wrapping (the release build's)
    return t % ref == 0u ? t : (t / ref + 1u) * ref;
}

// SourceCamera -> the divisor of adder_video_player.rs:184-203; 0.0 for the cameras that are todo!() there
ADDER_PLAYER_HD double player_max_intensity(uint32_t source_camera) {
    switch (source_camera) {
    case 0u: return 255.0;                    // FramedU8
    case 1u: return 65535.0;                  // FramedU16
    case 2u: return 4294967295.0;             // FramedU32
    case 3u: return 18446744073709551616.0;   // FramedU64: u64::MAX as f64
    case 6u: return 255.0;                    // Dvs
    case 7u: return 255.0;                    // DavisU8
    default: return 0.0;                      // FramedF32, FramedF64, Atis, Asint, unknown
    }
}

// (event_to_intensity(event) * ref_interval as f64) / M: a division, a multiplication, a division, in that order
ADDER_PLAYER_HD double player_value(uint32_t d, uint32_t t, double ref_f, double m) {
    double p = 0.0;  // D_SHIFT_F64[128]
    if (d < 128u) {
        union { uint64_t u; double f; } b;
        b.u = (uint64_t)(1023u + d) << 52;
        p = b.f;
    }
    const double in = t == 0u ? p : p / (double)t;
    return (in * ref_f) / m;
}

ADDER_PLAYER_HD uint8_t player_to_u8(double v) {  // saturate(rint(v * 255)), ties to even
    const double r = __builtin_rint(v * 255.0);
    return r >= 255.0 ? (uint8_t)255 : r > 0.0 ? (uint8_t)r : (uint8_t)0;
}

// The marks of n checks on the host, by the prefix-minimum form above (adder_player_schedule_host).
inline void player_schedule_marks(const uint32_t *cur_before, uint64_t n, uint64_t f0, uint64_t fl, uint8_t *marks) {
    int64_t pmin = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t stop = player_stop(cur_before[i], fl);
        marks[i] = player_frame_count(f0, i, pmin) < stop ? 1u : 0u;
        const int64_t term = player_term(stop, f0, i);
        pmin = i == 0u || term < pmin ? term : pmin;
    }
}

}  // namespace adder
