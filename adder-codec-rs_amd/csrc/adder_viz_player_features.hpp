// adder_viz_player_features.hpp -- where the pop schedule meets feature detection in the adder-viz player
// (include/adder_viz_player.h, "Feature detection"), shared by the kernels of adder_viz_player.hip and the host
// (adder_viz_features_host, adder_viz_overlay_host).
//
// Whether an event is a FAST corner depends on its unit's chain and the plane alone (adder_framer_features.hpp).  The
// schedule enters in three places:
//   - `consume` starts every period with last_event = None (adder.rs:409): the event after a pop is never tested;
//   - a feature is filed under the frames_written of the period its event lies in (driver.rs:497-506);
//   - the crosses of the interval popped with frame k are painted into running_frame after that frame's Some values
//     (adder.rs:359-388) and stay until a later Some overwrites them.
// pops[k] is the call-local index of the event after which frame w0 + k is popped (-1: before the call's first event),
// non-decreasing in k.
#pragma once
#include <stdint.h>

#include "adder_viz_player_logic.hpp"

namespace adder {

// #{k : pops[k] < i}: the pops that came before event i was ingested
ADDER_VIZ_HD uint32_t viz_pops_before(const int32_t *pops, uint32_t n_pops, int64_t i) {
    uint32_t lo = 0u, hi = n_pops;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if ((int64_t)pops[mid] < i)
            lo = mid + 1u;
        else
            hi = mid;
    }
    return lo;
}

// Event i is the first one of a `consume`: some frame was popped right after event i - 1 (for i == 0: at the opening
// of the call, after set_buffer_limit)
ADDER_VIZ_HD bool viz_period_start(const int32_t *pops, uint32_t n_pops, int64_t i) {
    const uint32_t k = viz_pops_before(pops, n_pops, i - 1);
    return k < n_pops && (int64_t)pops[k] == i - 1;
}

// A cross stamp: unit u takes 255 in the running frame right after the call's k-th popped frame was applied.  The
// call's stamps are sorted by (u, k); duplicates are allowed.
ADDER_VIZ_HD unsigned long long viz_stamp_key(uint32_t u, uint32_t k) { return ((unsigned long long)u << 32) | k; }

// the first stamp of unit u (or of a later unit)
ADDER_VIZ_HD uint32_t viz_stamp_first(const unsigned long long *stamps, uint32_t n, uint32_t u) {
    const unsigned long long key = viz_stamp_key(u, 0u);
    uint32_t lo = 0u, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (stamps[mid] < key)
            lo = mid + 1u;
        else
            hi = mid;
    }
    return lo;
}

// Is (u, k) stamped?  q is the unit's cursor: at viz_stamp_first(u) before frame 0, asked for k = 0, 1, .. in order.
ADDER_VIZ_HD bool viz_stamp_take(const unsigned long long *stamps, uint32_t n, uint32_t &q, uint32_t u, uint32_t k) {
    const unsigned long long key = viz_stamp_key(u, k);
    bool hit = false;
    while (q < n && stamps[q] <= key) {
        hit = hit || stamps[q] == key;
        ++q;
    }
    return hit;
}

// running_frame of one unit across one popped frame: Some overwrites, None keeps, then the cross wins
ADDER_VIZ_HD uint32_t viz_running_step(uint32_t cur, bool some, uint32_t v, bool stamped) {
    if (some) cur = v;
    if (stamped) cur = 255u;
    return cur;
}

}  // namespace adder
