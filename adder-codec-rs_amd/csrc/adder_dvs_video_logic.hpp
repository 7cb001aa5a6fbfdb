// adder_dvs_video_logic.hpp -- the arithmetic of the DVS event video and the event-count map (include/adder_dvs.h,
// adder-to-dvs/src/main.rs:195-239, 288, 382-411, 424-448) that host and device share.  No HIP: plain g++ compiles it
// (tests/cpu_sim/dvs_video_main.cpp).
//
// The reference keeps a deque of frames [F, E): F = frame_count, E = the exclusive end of the indices it covers (empty
// when E <= F).  Before it digests event i it makes one check, with cur_i = current_t (which never decreases):
//     pop_i = [cur_i > F_i * L + B];  frame F_i is emitted when pop_i and E_i > F_i;  F_{i+1} = F_i + pop_i
// (an empty deque pops nothing and F advances all the same: those indices are skipped).  Then event i may fire a DVS
// event at old_t + 1, frame g = (old_t + 1) / L; it is drawn iff g >= F_{i+1}, and then E = max(E, g + 1).
//
// The schedule.  Let T_i be the smallest F that stops the pop at position i:
//     T_i = 0 when cur_i <= B, else ceil((cur_i - B) / L)
// (F * L + B < cur  <=>  F < (cur - B) / L  <=>  F < ceil((cur - B) / L) for integers, L >= 1), so
// F_{i+1} = F_i + [F_i < T_i] = min(F_i + 1, max(F_i, T_i)): the recurrence of adder_player_logic.hpp with this T, and
// T never decreases because cur does not.  The proof there (adder_player_logic.hpp:4-15) uses nothing else, so it
// carries over word for word: with M_j = max(T_j, F_0),
//     F_{i+1} = min(F_0 + i + 1,  min_{j <= i} (M_j + i - j)),
// one inclusive prefix minimum of term_j = M_j - j.  F does not depend on E, so E follows from F: E_i is the running
// maximum of accept_j ? g_j + 1 : 0 over j < i, and the emitted frames are the pops with E_i > F_i.
//
// A frame's content does not depend on when it is popped: an event of frame g that comes after g's pop has g < F and is
// dropped, so frame g = blank + every accepted event of frame g, the last one in stream order winning.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ADDER_DVSV_HD __host__ __device__ __forceinline__
#else
#define ADDER_DVSV_HD inline
#endif

namespace adder {

// times, frame lengths and frame counts stay below 2^62 so that the signed terms of the prefix minimum cannot wrap
constexpr uint64_t kDvsVideoMax = 1ull << 62;

// a Rust `f32 as u128`: truncated, NaN and negatives give 0; clamped to 2^62 (above every time a stream reaches)
ADDER_DVSV_HD uint64_t dvs_video_ticks(float q) {
    if (!(q > 0.0f)) return 0u;
    return q >= 4611686018427387904.0f ? kDvsVideoMax : (uint64_t)q;
}

// (tps as f32 / fps) as u128
ADDER_DVSV_HD uint64_t dvs_video_frame_length(uint32_t tps, float fps) { return dvs_video_ticks((float)tps / fps); }

// (tps as f32 * buffer_secs) as u128
ADDER_DVSV_HD uint64_t dvs_video_buffer_ticks(uint32_t tps, float secs) { return dvs_video_ticks((float)tps * secs); }

// T: the smallest frame_count that stops the pop at a position whose current_t is `cur`; L >= 1
ADDER_DVSV_HD uint64_t dvs_video_stop(uint64_t cur, uint64_t L, uint64_t B) {
    if (cur <= B) return 0u;
    const uint64_t d = cur - B;
    const uint64_t q = d / L + (d % L != 0u ? 1u : 0u);
    return q > kDvsVideoMax ? kDvsVideoMax : q;
}

// term_i = max(T_i, F_0) - i; its inclusive prefix minimum is `pmin`
ADDER_DVSV_HD int64_t dvs_video_term(uint64_t stop, uint64_t f0, uint64_t i) {
    return (int64_t)(stop > f0 ? stop : f0) - (int64_t)i;
}

// F_i from pmin_{i-1} (unused at i == 0)
ADDER_DVSV_HD uint64_t dvs_video_frame_count(uint64_t f0, uint64_t i, int64_t pmin_before) {
    if (i == 0u) return f0;
    const uint64_t a = f0 + i;
    const uint64_t b = (uint64_t)((int64_t)(i - 1u) + pmin_before);
    return a < b ? a : b;
}

// a fired event's accept mark as the running maximum takes it: g + 1 when it is drawn, else 0
ADDER_DVSV_HD uint64_t dvs_video_reach(bool fired, uint64_t fire_t, uint64_t L, uint64_t f_after, bool draw) {
    if (!fired || !draw) return 0u;
    const uint64_t g = fire_t / L;
    return g >= f_after ? g + 1u : 0u;
}

// the count map's running maximum of the reference's wrapping u16 counter after `count` events of one unit
ADDER_DVSV_HD uint32_t dvs_video_count_peak(uint32_t count) { return count > 65535u ? 65535u : count; }

// ((count as u16) as f32 / m as f32 * 255.0) as u8: NaN (0 / 0) gives 0, the cast saturates
ADDER_DVSV_HD uint8_t dvs_video_count_byte(uint32_t count, uint32_t m) {
    const float v = ((float)(uint16_t)count / (float)m) * 255.0f;
    if (!(v > 0.0f)) return 0u;
    return v >= 255.0f ? (uint8_t)255 : (uint8_t)v;
}

struct DvsVideoState {
    uint64_t F, cur, E;
};

// One call of n events on the host, step by step as the kernels take it (every scan a running value here).
// pt[i]: the unit's time after event i (0: the unit's first event), fire_t[i]: old_t + 1 of a fired event (0: none).
// pop[i], accept[i]: marks (may be null); emitted[0 .. return value): the emitted frame indices, in order, as far as
// `cap` holds them.  *st is the carried state, replaced by the state after the call.
inline uint64_t dvs_video_schedule(const uint64_t *pt, const uint64_t *fire_t, uint64_t n, uint64_t L, uint64_t B,
                                   bool draw, DvsVideoState *st, uint8_t *pop, uint8_t *accept, uint64_t *emitted,
                                   uint64_t cap) {
    const uint64_t f0 = st->F;
    uint64_t cmax = 0, emax = 0, n_emit = 0, f_after = f0;
    int64_t pmin = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t cur = st->cur > cmax ? st->cur : cmax;  // before event i
        const uint64_t stop = dvs_video_stop(cur, L, B);
        const uint64_t f = dvs_video_frame_count(f0, i, pmin);
        const uint64_t e = st->E > emax ? st->E : emax;
        const bool p = f < stop;
        if (p && e > f) {
            if (n_emit < cap) emitted[n_emit] = f;
            ++n_emit;
        }
        f_after = f + (p ? 1u : 0u);
        const uint64_t reach = dvs_video_reach(fire_t[i] != 0u, fire_t[i], L, f_after, draw);
        if (pop) pop[i] = p ? 1u : 0u;
        if (accept) accept[i] = reach != 0u ? 1u : 0u;
        const int64_t term = dvs_video_term(stop, f0, i);
        pmin = i == 0u || term < pmin ? term : pmin;
        cmax = pt[i] > cmax ? pt[i] : cmax;
        emax = reach > emax ? reach : emax;
    }
    st->F = f_after;
    st->cur = st->cur > cmax ? st->cur : cmax;
    st->E = st->E > emax ? st->E : emax;
    return n_emit;
}

// The stream's end: one more check, then the tail [F, E), or one blank frame F when the deque is empty.
// Returns the number of frames; they are first .. first + count - 1.  *st becomes the state after the final check.
inline uint64_t dvs_video_finish(uint64_t L, uint64_t B, DvsVideoState *st, uint64_t *first) {
    uint64_t n = 0;
    *first = st->F;
    if (st->F < dvs_video_stop(st->cur, L, B)) {
        if (st->E > st->F) n = 1;
        st->F += 1u;
    }
    if (st->E <= st->F) {
        if (n == 0u) *first = st->F;
        // an emitted frame F - 1 is followed by the blank frame F: contiguous as well
        return n + 1u;
    }
    return n + (st->E - st->F);
}

}  // namespace adder
