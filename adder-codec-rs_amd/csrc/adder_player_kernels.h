// adder_player_kernels.h -- between adder_player_api.cpp and adder_player.hip (include/adder_player.h is the public side).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace adder {


struct PlayerScalars {  // device words of one call, read back once the schedule is known
    unsigned long long bad;    // smallest index of an event outside the plane (UINT64_MAX: none)
    unsigned long long eof;    // index of the first EOF / undecodable wire record (n: none)
    unsigned long long total;  // frames the call shows (the required frame count)
    unsigned long long cur;    // current_t after the call's applied events
};

struct PlayerArgs {
    uint32_t width, height, channels, units;
    uint32_t key_bits;   // radix bits of a unit key; key `units` marks a record that takes part in nothing
    uint32_t absolute;   // 1: AbsoluteT rules, 0: the accumulating rules of every other time mode
    uint32_t ref;        // ref_interval
    int32_t out_type;
    double ref_f;        // ref_interval as f64
    double m;            // the source camera's maximum intensity
    uint64_t fl;         // frame length in ticks, clamped to 2^32
    // per-unit state
    uint32_t *last_ts;
    double *display;
    uint32_t *run_lo;    // units + 1: where each unit's run starts in the call's sorted order
};

struct PlayerScratch {  // per call; n entries unless said otherwise
    uint32_t *keys0, *keys1, *idx0, *idx1;
    double *s_val;     // sorted order: the event's display value
    uint32_t *s_ts;    // sorted order: the unit's last_ts after the event
    uint32_t *cand;    // n + 1: [0] the carried current_t, [i + 1] event i's candidate for current_t (0: none)
    uint32_t *cur;     // n + 1: current_t before check i (inclusive prefix maximum of cand)
    int64_t *term;     // n + 1: max(T_i, F_0) - i
    int64_t *pmin;     // n + 1: its inclusive prefix minimum
    uint8_t *mark;     // n + 1: check i shows a frame
    uint32_t *offs;    // n + 1: exclusive scan of mark
    uint32_t *pos;     // n + 1: the display positions s_0 < s_1 < ...
    void *temp;
    size_t temp_bytes;
    PlayerScalars *sc;
    const uint32_t *keys, *idx;  // the sorted arrays, set by player_schedule
};

size_t player_temp_bytes(uint64_t n);
// n <= INT32_MAX - 1.  Queues keys, sort, values, clock and display schedule on `stream`; `final_check`: the call
// makes one check after its last event.  The caller reads PlayerScalars afterwards.
hipError_t player_schedule(const PlayerArgs &a, int source, const void *d_in, uint64_t n, int final_check,
                           uint32_t cur0, uint64_t f0, PlayerScratch &s, hipStream_t stream);
// Writes the n_frames frames of the schedule to d_frames, then commits the state of the events before `lim`.
hipError_t player_handout(const PlayerArgs &a, uint64_t n, uint64_t lim, uint64_t n_frames, void *d_frames,
                          const PlayerScratch &s, hipStream_t stream);
hipError_t player_display(const PlayerArgs &a, void *d_frame, hipStream_t stream);

}  // namespace adder
