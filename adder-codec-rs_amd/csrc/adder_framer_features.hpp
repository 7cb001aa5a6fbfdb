// adder_framer_features.hpp -- per-event logic of feature detection while framing (Framer::ingest_event with
// detect_features on, adder-codec-rs/src/framer/driver.rs:446-553; is_feature, utils/cv.rs:56-212).
//
// The reference runs FAST 9_16 on one mutable plane inside a serial loop over the stream: event i sees the ring
// pixels as they stood after event i - 1.  Everything an event contributes follows from its own unit's chain:
//   val8     the unit's last_frame_intensity after the event, `Into<f64> as u8` (saturating; driver.rs:487-489),
//            written for EVERY event (D_EMPTY, no frame crossed, AbsoluteT event from the pixel's past);
//   t_after  the t the player carries forward as last_event.t: ingest_event_for_chunk overwrites event.t when the
//            event sets an intensity in an AbsoluteT stream outside the SAE view (driver.rs:1022-1028).
// A ring pixel's value at event i is then the val8 of that pixel's last event with an index below i, or the
// plane carried from the previous call.  Compiled for the device and, by tests/cpu_sim, for the host.
#pragma once
#include <stdint.h>

#include "adder_framer.hpp"

namespace adder {

struct FramerFeatureStep {
    bool fills;        // frames (from, to] take the unit's intensity (framer_step)
    int32_t from, to;
    bool overflow;
    uint32_t val8;     // running_intensities[y][x][c] after the event
    uint32_t t_after;  // event.t as ingest_event_for_chunk leaves it
};

// framer_step plus what detection adds for the event (d, t) of the unit whose trackers are p
ADDER_HD FramerFeatureStep framer_feature_step(FramerPx &p, uint32_t d, uint32_t t, const FramerConsts &k) {
    FramerFeatureStep o;
    o.from = o.to = 0;
    o.overflow = false;
    const uint32_t pr = (uint32_t)p.ts;  // prev_running_ts as u32
    o.fills = framer_step(p, d, t, k, o.from, o.to, o.overflow);
    o.t_after = t;
    if (o.fills && d != 255u && k.abs_t && k.view_mode != kViewSae) o.t_after = t > pr ? t - pr : 0u;
    o.val8 = p.lasti > 255u ? 255u : p.lasti;  // <T as Into<f64>>::into(..) as u8
    return o;
}

// cv.rs:25-30 CIRCLE3[k] as (dx, dy)
ADDER_HD int fast_ring_dx(uint32_t k) { return (int)((0x2100012345666543ull >> (4u * k)) & 0xfu) - 3; }
ADDER_HD int fast_ring_dy(uint32_t k) { return (int)((0x6543210001234566ull >> (4u * k)) & 0xfu) - 3; }

// THRESHOLD_TABLE (cv.rs:35-50): 1 darker than centre - 30, 2 brighter than centre + 30
ADDER_HD uint32_t fast_class(int p, int c) { return p < c - kFastThreshold ? 1u : p > c + kFastThreshold ? 2u : 0u; }

// is_feature past its border / channel check, on ring values that cost something to get: ring(k) is asked for
// CIRCLE3[k] once at most.  The four opposite pairs 0/8, 2/10, 4/12, 6/14 come first with the reference's rejects
// (cv.rs:86-117; `d` only loses bits, so leaving as soon as it is 0 answers the same); whoever survives gathers the
// other eight and takes the arc test of fast9_is_feature.
template <class Ring>
ADDER_HD bool fast9_ring_is_feature(int centre, Ring ring) {
    int v[16];
    uint32_t d = 3u;
#pragma unroll
    for (uint32_t k = 0; k < 8u; k += 2u) {
        v[k] = ring(k);
        v[k + 8u] = ring(k + 8u);
        d &= fast_class(v[k], centre) | fast_class(v[k + 8u], centre);
        if (d == 0u) return false;
    }
#pragma unroll
    for (uint32_t k = 1; k < 8u; k += 2u) {
        v[k] = ring(k);
        v[k + 8u] = ring(k + 8u);
    }
    uint32_t bright = 0u, dark = 0u;
#pragma unroll
    for (uint32_t k = 0; k < 16u; ++k) {
        const uint32_t cl = fast_class(v[k], centre);
        dark |= (cl & 1u) << k;
        bright |= (cl >> 1) << k;
    }
    return fast_arc9(bright) || fast_arc9(dark);
}

// the same on 16 gathered values, ring[k] = the pixel at CIRCLE3[k]
ADDER_HD bool fast9_ring16_is_feature(int centre, const uint8_t *ring16) {
    return fast9_ring_is_feature(centre, [ring16](uint32_t k) { return (int)ring16[k]; });
}

// Is event (x, y, c, t) looked at?  driver.rs:491-492 (`last_event` is Some and time != last.t) and the head of
// is_feature (cv.rs:61: 3 pixels from the border, channel 0 or None).
ADDER_HD bool framer_feature_is_candidate(uint32_t x, uint32_t y, uint32_t c, uint32_t t, bool last_valid,
                                          uint32_t last_t, uint32_t w, uint32_t h) {
    if (!last_valid || t == last_t) return false;
    if (!(c == 0u || c == 0xffu)) return false;
    return !(x < kFastBorder || x + kFastBorder >= w || y < kFastBorder || y + kFastBorder >= h);
}

// The value of a unit at event i: idx[lo, hi) are the input indices of the unit's events of this call, ascending;
// the last one below i counts, else the plane value carried into the call.
ADDER_HD uint32_t framer_feature_value_before(const uint32_t *idx, const uint8_t *val8_sorted, uint32_t lo, uint32_t hi,
                                              uint32_t i, uint32_t carried) {
    const uint32_t lo0 = lo;
    while (lo < hi) {  // first position whose index is >= i
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (idx[mid] < i) lo = mid + 1u;
        else hi = mid;
    }
    return lo > lo0 ? (uint32_t)val8_sorted[lo - 1u] : carried;
}

}  // namespace adder
