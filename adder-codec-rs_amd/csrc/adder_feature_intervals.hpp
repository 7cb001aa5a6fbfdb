// adder_feature_intervals.hpp -- FrameSequence::features, the deque of FeatureIntervals (driver.rs:252-257), as the
// host keeps it for the framer (adder_framer_api.cpp) and the adder-viz player (adder_viz_player_api.cpp): filing one
// feature (driver.rs:497-549) and pop_features (:851-873).  Restated, not fixed: the u32 arithmetic on `time` wraps as
// the reference's release build does.  Where the reference would index past the deque and panic, or grow it by more
// than 2^22 intervals for one feature, that feature and every later one is not filed (`broken`, with `err`).
#pragma once
#include <stdint.h>

#include <cstdio>
#include <deque>
#include <string>
#include <vector>

namespace adder {

struct FeatureInterval {
    uint64_t end_ts;
    std::vector<uint16_t> xy;  // {x, y} pairs
};

struct FeatureIntervals {
    std::deque<FeatureInterval> dq;
    bool broken = false;  // the reference would have panicked
    std::string err;

    void clear() {
        dq.clear();
        broken = false;
        err.clear();
    }

    // driver.rs:497-549 for one feature found at `time`, under the frames_written its event was ingested with
    void file(uint32_t tpf, uint32_t time, uint16_t x, uint16_t y, int64_t frames_written) {
        if (broken) return;
        size_t idx = (int64_t)(time / tpf) >= frames_written ? (size_t)(uint32_t)(time / tpf - (uint32_t)frames_written) : 0u;
        if (time % tpf == 0u && idx > 0u) idx -= 1u;
        auto fail = [&](const char *why) {
            char buf[256];
            snprintf(buf, sizeof buf, "the feature at t = %u (%u, %u) %s (frames_written %lld, %zu intervals): it and every "
                     "later feature is not filed", time, x, y, why, (long long)frames_written, dq.size());
            broken = true;
            err = buf;
        };
        if (idx >= dq.size()) {
            if (dq.empty()) {
                dq.push_back({(uint64_t)tpf, {}});
                dq.push_back({(uint64_t)tpf * 2u, {}});
            }
            const uint64_t new_end_ts = time % tpf == 0u ? time : (uint32_t)((time / tpf + 1u) * tpf);  // u32, wrapping
            uint64_t running_end_ts = dq.back().end_ts + tpf;
            if (running_end_ts <= new_end_ts && (new_end_ts - running_end_ts) / tpf >= (1u << 22))
                return fail("would grow the interval deque by more than 2^22 intervals");
            while (running_end_ts <= new_end_ts) {
                dq.push_back({running_end_ts, {}});
                running_end_ts += tpf;
            }
        }
        if (idx >= dq.size()) return fail("lies past the interval deque, where the reference panics");
        if (dq[idx].end_ts < (uint64_t)time) dq[idx].end_ts = time;  // detection switched on late (:544-547)
        dq[idx].xy.push_back(x);
        dq[idx].xy.push_back(y);
    }

    // the number of {x, y} pairs pop() would hand out
    size_t front_pairs() const { return dq.empty() ? 0u : dq.front().xy.size() / 2u; }

    // driver.rs:851-873
    FeatureInterval pop(uint32_t tpf) {
        if (dq.empty()) {
            dq.push_back({(uint64_t)tpf, {}});
            dq.push_back({(uint64_t)tpf * 2u, {}});
        } else {
            dq.push_back({(uint64_t)tpf + dq.back().end_ts, {}});
        }
        FeatureInterval f = std::move(dq.front());
        dq.pop_front();
        return f;
    }
};

}  // namespace adder
