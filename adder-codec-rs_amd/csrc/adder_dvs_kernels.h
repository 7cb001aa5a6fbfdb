// adder_dvs_kernels.h -- between adder_dvs_api.cpp and adder_dvs.hip (include/adder_dvs.h is the public side).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace adder {


struct DvsScalars {  // device words of one call, read back once at its end
    unsigned long long bad;  // smallest index of a bad event (UINT64_MAX: none)
    unsigned long long eof;  // index of the first EOF / undecodable wire record (n: none)
    unsigned long long total;  // fired events of the call (the required output count)
};

struct DvsArgs {
    uint32_t width, height, channels, units;
    uint32_t key_bits;     // radix bits of a unit key; key `units` marks an event that is never walked
    uint32_t delta_t;      // 1: DeltaT accumulation, 0: AbsoluteT rules
    uint32_t framed;       // is_framed(source_camera): times rounded up to ref_interval
    uint64_t ref;          // ref_interval
    double ref_f;          // ref_interval as f64
    double win_hi;         // ln_1p(1.0) - theta
    double win_lo;         // ln_1p(0.0) + theta
    double half;           // theta / 2.0
    // per-unit state: `cur` is read, a call's walk writes `nxt`, the commit copies the walked units back
    uint8_t *cur_init, *nxt_init;
    double *cur_ln, *nxt_ln;
    uint64_t *cur_t, *nxt_t;
};

struct DvsScratch {  // per call, n entries each unless said otherwise
    uint32_t *keys0, *keys1, *idx0, *idx1;
    double *s_ln;      // sorted order: the event's ln intensity
    uint64_t *s_td;    // sorted order: raw t | d << 32
    uint8_t *flag;     // input order: 0 none, 1 negative, 2 positive
    uint64_t *tout;    // input order: the fired event's time
    uint32_t *offs;    // input order: exclusive scan of flag != 0
    void *temp;
    size_t temp_bytes;
    DvsScalars *sc;
};

// ---- the event video and the count map (adder_dvs_video.hip), only on a context that enabled them ----
struct DvsVideoScalars {  // device words of one call's video arm
    unsigned long long F, E, cur;  // the carried state after the call
    unsigned long long n_emit;     // frames the call emitted (their indices are in DvsVideoArgs::list)
    unsigned long long need;       // ring slots the call needs: E - lo
    unsigned long long ok;         // 1: the DVS output and the ring both fit, the call is committed
};

struct DvsVideoArgs {
    uint64_t L, B;            // frame length and buffer, in ticks; L >= 1
    uint64_t F0, E0, cur0;    // the carried state before the call
    uint64_t lo;              // the lowest frame index that holds a ring slot (the oldest unpopped frame, else F0)
    uint64_t ring_frames;
    uint32_t draw;
    uint8_t *ring;            // [ring_frames][h][w], frame f in slot f % ring_frames; 128 outside [lo, E)
    uint32_t *cur_cnt, *nxt_cnt;  // per unit: committed events, under the cur / nxt discipline of DvsArgs
    // per call, n entries each
    uint64_t *pt;     // input order: the unit's time after the event (0: a unit's first event, or not walked)
    int64_t *term;    // the schedule's terms, then their prefix minimum
    uint64_t *reach;  // accept ? g + 1 : 0, then its prefix maximum
    uint8_t *mark;    // 1: the position's pop emits a frame
    uint32_t *moffs;  // exclusive scan of mark
    uint64_t *list;   // the emitted frame indices
    uint64_t *k0, *k1;  // draw: sort keys (frame - lo) * w * h + y * w + x
    uint32_t *v0, *v1;  // draw: sort values, the event's input index
    void *temp;
    size_t temp_bytes;
    DvsVideoScalars *vs;
};

size_t dvs_video_temp_bytes(uint64_t n);
// after the walk and the scatter: the schedule of the call's positions, its emitted frames and its verdict (vs->ok)
hipError_t dvs_video_schedule(const DvsArgs &a, const DvsVideoArgs &va, uint64_t n, uint64_t out_cap,
                              const DvsScratch &s, hipStream_t stream);
// after the commit: the accepted events into the ring, the last one in stream order winning
hipError_t dvs_video_draw(const DvsArgs &a, const DvsVideoArgs &va, int source, const void *d_in, uint64_t n,
                          const DvsScratch &s, hipStream_t stream);
// k ring frames (indices d_list[0 .. k)) densely into d_out; their slots are refilled with 128
hipError_t dvs_video_handout(const DvsArgs &a, const DvsVideoArgs &va, const uint64_t *d_list, uint64_t k,
                             uint8_t *d_out, hipStream_t stream);
// [h][w][3] bytes; d_m: one scratch word
hipError_t dvs_video_count_map(const DvsArgs &a, const uint32_t *d_cnt, uint32_t *d_m, uint8_t *d_out,
                               hipStream_t stream);

size_t dvs_temp_bytes(uint64_t n);
// n <= INT32_MAX.  Queues the whole conversion on `stream`; the caller reads DvsScalars afterwards.  va: null unless
// the context's video is enabled (then DvsVideoScalars is read as well).
hipError_t dvs_convert(const DvsArgs &a, int source, const void *d_in, uint64_t n, int out_format, void *d_out,
                       uint64_t out_cap, const DvsScratch &s, hipStream_t stream, const DvsVideoArgs *va = nullptr);
size_t dvs_sort_temp_bytes(uint64_t n);
// stable sort of n records by 32-bit t; keys / vals: 2 * n uint32 each, tmp: n records
hipError_t dvs_sort(void *d_records, uint64_t n, int out_format, uint32_t *keys0, uint32_t *keys1, uint32_t *vals0,
                    uint32_t *vals1, void *tmp, void *temp, size_t temp_bytes, hipStream_t stream);
hipError_t dvs_log1p_run(const double *d_x, double *d_y, uint64_t n, hipStream_t stream);

}  // namespace adder
