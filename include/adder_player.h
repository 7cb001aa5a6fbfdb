/* adder_player.h -- C-ABI of the latest-event video player (libadder_hip.so).
 *
 * The reference's adder_video_player (adder-codec-rs/src/bin_cv/adder_video_player.rs:52-216) on the device: it
 * "simply displays the intensity of the most recently fired event for each pixel" and shows the matrix each time the
 * stream's clock passes a playback-frame boundary.  No per-pixel frame queue, one value per unit.
 *
 * State.  last_ts[unit] (u32, 0), display[unit] (f64, 0.0), the unit being (y, x, c) with `c = None` counted as 0;
 * current_t (u32, 0); frame_count (1); FL = (tps as f64 / playback_fps) as u128, the truncated integer (FL = 0 is
 * legal: a playback rate above tps; FL is clamped to 2^32, which changes nothing because current_t < 2^32).
 *
 * One loop iteration per record position, in stream order:
 *  1. the display check: if current_t > frame_count * FL (strict), the matrix as it stands is one output frame and
 *     frame_count += 1.  At most one frame per iteration.
 *  2. the next record is read.  An EOF record, a short read or an undecodable record ends the loop: the iteration
 *     that meets the end has already made its check, so a stream of N records has N + 1 checks.  Nothing is shown
 *     after the loop.
 *  3. a record with d > 128 (129..=255, D_EMPTY included) changes nothing; its iteration still made its check.
 *  4. otherwise, time.  AbsoluteT: current_t = max(current_t, t); dt = t - last_ts; last_ts = t rounded up to the
 *     next multiple of ref_interval unless it is one; the event's time becomes dt.  Every other time mode:
 *     last_ts += t; the same round-up; current_t = max(current_t, last_ts); the event's time stays t.  The round-up
 *     is unconditional, whatever the source camera (unlike the framer).  All u32 arithmetic wraps, as the
 *     reference's release build does; its debug build panics instead.
 *  5. value: I = 2^d as f64 when the event's time is 0, else 2^d / time (2^128 counts as 0.0);
 *     display[unit] = (I * ref_interval as f64) / M, M = 255 for FramedU8 / Dvs / DavisU8, 65535 for FramedU16,
 *     4294967295 for FramedU32, u64::MAX as f64 for FramedU64: one division, one multiplication and one division
 *     in binary64, in that order.  The other cameras are todo!() in the reference and refused at create.
 * Not reproduced: the progress line, the wall-clock wait, the window, show_display_force's resize to 940 rows.  The
 * output frame is the matrix handed to show_display_force.
 *
 * Errors, as this library defines them (the reference indexes out of bounds and panics): an event with d <= 128
 * outside the plane at batch index b commits the batch exactly as if it had ended before b, returns
 * ADDER_PLAYER_E_BAD_EVENT with b in *bad_index and applies nothing after it.  A call whose frames do not fit
 * returns ADDER_E_OUT_CAPACITY with the needed count in *n_frames and changes nothing.
 *
 * Splitting.  Any split of a stream into calls gives the same frames as one call, the same final matrix and clock;
 * empty calls are allowed.  A play call makes the check before each of its records; the stream's last check is made
 * by the wire call that meets the EOF record, or by adder_player_finish for the AdderEvent form.
 *
 * Frames are [height][width][channels] planes of out_type.  ADDER_PLAYER_F64 is the reference's matrix bit for bit.
 * ADDER_PLAYER_U8 is saturate(rint(v * 255)), ties to even: OURS, the scaling OpenCV's imshow applies to a floating
 * matrix, which the reference's own text does not contain.  Frame buffers must be 8-byte aligned. */
#ifndef ADDER_PLAYER_H
#define ADDER_PLAYER_H

#include <stddef.h>
#include <stdint.h>

#include "adder_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ADDER_PLAYER_ABI_VERSION 1u
#define ADDER_PLAYER_E_BAD_EVENT (-16)
#define ADDER_PLAYER_NO_BAD_EVENT UINT64_MAX

enum { ADDER_PLAYER_F64 = 0, ADDER_PLAYER_U8 = 1 };

typedef struct AdderPlayerParams {
    uint32_t abi_version; /* = ADDER_PLAYER_ABI_VERSION */
    uint16_t width;
    uint16_t height;
    uint8_t channels;       /* 1 or 3 */
    uint8_t time_mode;      /* ADDER_TIME_ABSOLUTE_T (1) or anything else (the accumulating rules) */
    uint16_t reserved0;
    uint32_t ref_interval;  /* > 0 */
    uint32_t tps;           /* ticks per second */
    uint32_t source_camera; /* SourceCamera index: 0..3, 6, 7; the others are refused */
    double playback_fps;    /* finite, > 0 (the reference's CLI default: 60.0) */
    int32_t out_type;       /* ADDER_PLAYER_F64 or ADDER_PLAYER_U8 */
    int32_t device_id;
} AdderPlayerParams;

typedef struct AdderPlayer AdderPlayer;

/* Fills `p` (playback_fps = 60.0, F64, device 0) from the header of a raw .adder stream of codec version 0..3.
 * *header_bytes = where the events start, *event_bytes = 9 (one channel) or 11. */
int adder_player_parse_header(const uint8_t *buf, size_t len, AdderPlayerParams *p, uint32_t *header_bytes,
                              uint32_t *event_bytes);

int adder_player_create(const AdderPlayerParams *p, AdderPlayer **out);
void adder_player_destroy(AdderPlayer *pl);
/* Back to the start of a stream: last_ts 0, display 0.0, current_t 0, frame_count 1. */
int adder_player_reset(AdderPlayer *pl);
/* Describes the last failure of `pl` (or of the last failed create when pl is null). */
const char *adder_player_last_error(const AdderPlayer *pl);

/* n AdderEvents (device, stream order): the display check before each of them, then the event.  The frames shown go
 * to d_frames[0 .. *n_frames); frame_cap counts frames.  *bad_index = the index of the bad event within this batch,
 * or ADDER_PLAYER_NO_BAD_EVENT.  Waits for `stream`. */
int adder_player_play_device(AdderPlayer *pl, const AdderEvent *d_events, uint64_t n, void *d_frames,
                             uint64_t frame_cap, uint64_t *n_frames, uint64_t *bad_index, void *stream);
/* The same for n_records raw wire records (the 9 / 11-byte big-endian body of a .adder file).  An EOF record
 * (x == y == 0xFFFF) or an undecodable one ends the stream there and the call makes the stream's last check itself:
 * *n_consumed = the records before it (n_records when there is none).  Records after it are not looked at. */
int adder_player_play_wire_device(AdderPlayer *pl, const uint8_t *d_wire, uint64_t n_records, void *d_frames,
                                  uint64_t frame_cap, uint64_t *n_frames, uint64_t *bad_index, uint64_t *n_consumed,
                                  void *stream);
/* The pending last check of a stream played through the AdderEvent form, which has no EOF record: at most one frame
 * (device memory). */
int adder_player_finish(AdderPlayer *pl, void *d_frames, uint64_t frame_cap, uint64_t *n_frames, void *stream);
/* Host-pointer forms of the two play calls: copy in, play on the device, copy the frames out. */
int adder_player_play_host(AdderPlayer *pl, const AdderEvent *events, uint64_t n, void *frames, uint64_t frame_cap,
                           uint64_t *n_frames, uint64_t *bad_index);
int adder_player_play_wire_host(AdderPlayer *pl, const uint8_t *wire, uint64_t n_records, void *frames,
                                uint64_t frame_cap, uint64_t *n_frames, uint64_t *bad_index, uint64_t *n_consumed);

/* The matrix as it stands now, in out_type, without a check: what a caller shows between batches. */
int adder_player_display_device(AdderPlayer *pl, void *d_frame, void *stream);
int adder_player_display(AdderPlayer *pl, void *frame);
int adder_player_clock(const AdderPlayer *pl, uint32_t *current_t, uint64_t *frame_count);

/* The display schedule on the host, for self-tests: marks[i] = 1 when check i of n shows a frame, given current_t
 * before each check (non-decreasing), the carried frame_count f0 and the frame length fl.  The same arithmetic the
 * kernels use (a prefix minimum, not the serial loop). */
void adder_player_schedule_host(const uint32_t *cur_before, uint64_t n, uint64_t f0, uint64_t fl, uint8_t *marks);
/* (tps as f64 / playback_fps) as an integer, clamped to 2^32. */
uint64_t adder_player_frame_length(uint32_t tps, double playback_fps);

#ifdef __cplusplus
}
#endif
#endif /* ADDER_PLAYER_H */
