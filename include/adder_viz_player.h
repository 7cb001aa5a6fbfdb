/* adder_viz_player.h -- C-ABI of the adder-viz player (libadder_hip.so): a FrameSequence<u8> with one row per chunk
 * and a buffer limit, popped the way the reference's interactive player pops it.
 *
 * The reference: adder-viz/src/player/adder.rs:319-440 (`consume`) over adder-codec-rs/src/framer/driver.rs:437-562
 * (ingest_event), 632-677 (flush_frame_buffer), 828-843 (is_frame_0_filled), 878-925 (pop_next_frame), 984-1133
 * (ingest_event_for_chunk).  The framer is FramerBuilder::new(plane, 1) -- every row is its own chunk --
 * INSTANTANEOUS, Some(fps), buffer_limit = Some(60) by default.  It sits between the exact framer (adder_framer.h,
 * which waits for the slowest pixel) and the latest-event player (adder_player.h, no frame queue): exact frames while
 * every pixel keeps up, a forced, partly empty frame once some pixel runs more than buffer_limit frames ahead.  An
 * event that arrives after its frame was popped is dropped for that frame, so WHEN frames are popped decides what they
 * hold: the pop schedule below is reproduced, not sidestepped.  Restated, not fixed.
 *
 * Per event.  The per-unit step is the framer's (csrc/adder_framer.hpp, framer_step): the clock and its round-up for
 * framed cameras, the fill range (from, to], the value (D_EMPTY repeats the last intensity), every view arm for u8.
 * An AbsoluteT event from the unit's past (prev_ts >= t) changes nothing and takes no part in anything below.  Every
 * other event is "checked": it has a global stream index i (counted from the context's creation), a row r_i, and
 * L_i, the unit's last_filled after the event.
 *
 * The pop schedule.  W = frames_written, limit = the buffer limit, s = the index of the first event ingested while
 * frames_written == W.
 *   Row state.  A row's chunk_filled_tracker entry always equals "frame W of this row is complete or forced"; only the
 *     row's own events and pops change it.
 *   nat_r(W): the index of the event that gives frame W of row r its last missing unit; -inf when the row is complete
 *     before s, +inf while a unit is missing.  An event that covers W always arrives in time to count, because W has
 *     not been popped.
 *   forced_r(W, s): the first checked event i >= s of row r with L_i > W + limit; +inf without a limit.  An event from
 *     before s never forces: the forcing sets filled_count of the then-current frame 0 only.
 *   End of the period.  E_W = max over rows of min(nat_r(W), forced_r(W, s)).  ingest_event returns true at event E_W
 *     and at no earlier event of the period.  While E_W is +inf the period stays open across calls.
 *   The pops at E_W.  Frame W is popped.  Then, with M the largest L of any event <= E_W since creation, W <- W + 1 and
 *     the pop repeats while (a) limit is set and max(M, W) - W + 1 > limit -- the `chunk.len() > buffer_limit` clause
 *     of is_frame_0_filled: a row's deque length is max(maxL_r, W) - W + 1 -- or (b) every row's frame W is complete
 *     by events <= E_W.
 *   The next period begins at s = E_W + 1.
 *   Content.  In the frame j popped after event E, unit u is Some(v) if the one event of u whose fill range contains j
 *     has index <= E; v is the unit's last intensity after that event.  Otherwise u is None: the event was late and is
 *     dropped for j, or no event covered j.
 *   running_frame: zero at creation; for each popped frame Some overwrites the unit, None keeps it (adder.rs:342-356).
 *
 * The end of the stream, adder_viz_player_finish: the Err arm of `consume`, where flush_frame_buffer and the consume
 * recursion alternate.  While M > W: the Nones of frame W are filled with each unit's current last_frame_intensity
 * (the unit's latest value, even one from a later frame: the reference's quirk, reproduced), frame W is popped, then
 * the pops repeat as above with E = the last event of the stream; frames popped by that repetition keep their Nones.
 * Frame M is never shown.  A context that was finished takes no more events.
 *
 * OURS, stated as ours:
 *   - limit == 0 is refused (create, set_buffer_limit): the reference's `while is_frame_0_filled()` never ends there,
 *     a deque always holds at least one frame.
 *   - no limit (has_buffer_limit = 0) is allowed: the exact framer's frames, popped at the player's positions.
 *   - pops happen right after the event that completed the period (nothing lies between that event and the next
 *     `consume`), so any split of a stream into calls gives the same frames; empty calls are allowed.
 *   - adder_viz_player_set_buffer_limit between calls is adaptive_state_update: the `while` loop of adder.rs:339 runs
 *     at the start of the next call (or finish) with the new limit.  Without it a call opens with no such loop (the
 *     reference runs it only after a `consume` returned, and those pops were made right after that event).
 *   - an event outside the plane at batch index b: the batch commits exactly as if it had ended before b, b is
 *     reported in *bad_index and the status is ADDER_VIZ_PLAYER_E_BAD_EVENT (the reference skips a row past the plane
 *     and indexes out of bounds otherwise).
 *   - frames that do not fit: ADDER_E_OUT_CAPACITY with the needed count in *n_frames, nothing changes.
 *   - a unit that runs ring_frames or more frames ahead of frames_written: ADDER_E_OUT_CAPACITY with *n_frames = 0 and
 *     the framer's message (raise ring_frames); nothing changes.
 *   - wire input stops at an EOF record (x == y == 0xFFFF) or an undecodable record: *n_consumed = the records before
 *     it; the caller then calls finish.
 *   - not built: u16 / u32 frames, compressed input, changing the view mid-stream.
 *
 * Feature detection (adder_viz_player_detect_features; adder.rs:281-282, 359-388 over driver.rs:482-553, 851-873).
 * With detection on every event writes running_intensities[y][x][c] = its unit's last intensity and, when its t differs
 * from the t ingest_event_for_chunk left in the previous event, is on channel 0 / None and 3 pixels off the border, is
 * tested with FAST 9_16 on the plane as it stands (adder_framer.h has the per-event rules).  None of that depends on
 * frames_written: an event that is late and dropped for its frame still writes the plane and is still tested.  The pop
 * schedule enters in three places:
 *   - `consume` sets last_event = None when it is entered (adder.rs:409): the first event of every period -- the event
 *     after each distinct P_j, and the first event after set_buffer_limit or detect_features -- is never tested.  It
 *     still writes the plane.
 *   - A feature is filed (driver.rs:497-549) under the frames_written of the period its event lies in, from the RAW
 *     event.t (a delta in a DeltaT stream: restated, not fixed), in u32 arithmetic that wraps.
 *   - Every popped frame takes one FeatureInterval (pop_features, adder.rs:359), detection on or off: the deque runs
 *     from creation.  Its features are painted into running_frame after the frame's Some values as crosses of 255:
 *     radius 2, the vertical and the horizontal arm, every channel of the pixel.  A cross wins over that frame's value
 *     and stays across later Nones until a Some overwrites it.  ADDER_VIZ_FRAME_RUNNING frames and
 *     adder_viz_player_running_frame carry the crosses (the context's running frame holds them whichever form a call
 *     asked for); ADDER_VIZ_FRAME_POPPED frames do not.
 * The carried last event is valid unless the previous call's last consumed event ended a period, the limit or
 * detection was set since, or the context was reset: any split of a stream into calls gives the same features,
 * intervals and frames.  A call that is refused (frames that do not fit, a unit past the ring) changes none of the
 * plane, the carried event, the deque and the crosses; a bad event at index b commits them as if the batch had ended
 * before b.  With detection on a call waits for its stream once more (to read the features back) and takes fewer
 * than 2^31 events, as without.  With detection never switched on every entry point launches what it launched before
 * this block existed.
 * Where the reference would index past the deque and panic, or grow it by more than 2^22 intervals for one feature,
 * that feature and every later one is not filed (adder_viz_player_features still lists them) and
 * adder_viz_player_frame_features reports ADDER_E_BAD_PARAMS with the reason from then on, its outputs still filled;
 * framing and the pops of intervals go on, adder_viz_player_reset clears the state.  The panic is reached where
 * (time / tpf + 1) * tpf wraps u32 while the unit stays inside the frame ring, i.e. for tpf > 2^32 / ring_frames: at
 * tpf 2^17 and ring_frames 65536 an event with t = 0xFFFFFFFF reaches frame 32767, its interval end wraps to 0, the
 * deque does not grow and the index lies past it.  Not reached through this interface: growth by 2^22 intervals (the
 * unit would be 2^22 frames ahead, the ring holds at most 65536: refused, nothing changes) and the raised end_ts of
 * driver.rs:544-547 (every pop takes an interval, so the deque's front always ends at (frames_written + 1) * tpf and
 * interval idx ends at or after `time`).
 * A call that fails with ADDER_E_HIP after its checks (an allocation, a copy or a launch inside the hand-out) leaves
 * the context unusable: destroy it.  Not built: EventCoordless frames, detection across row bands.
 *
 * Frames are [n][height][width][channels] u8 in one of two forms:
 *   ADDER_VIZ_FRAME_POPPED   the popped frame with None as 0: the bytes of the reference's write_frame_bytes;
 *   ADDER_VIZ_FRAME_RUNNING  the player's running_frame after the frame was applied.
 * pop_index (host memory, optional, room for frame_cap entries) receives P_j for each frame: the global index of the
 * event after which it was popped (-1: before the first event). */
#ifndef ADDER_VIZ_PLAYER_H
#define ADDER_VIZ_PLAYER_H

#include <stddef.h>
#include <stdint.h>

#include "adder_framer.h" /* AdderFramerFeature */
#include "adder_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ADDER_VIZ_PLAYER_ABI_VERSION 1u
#define ADDER_VIZ_PLAYER_E_BAD_EVENT (-16) /* = ADDER_PLAYER_E_BAD_EVENT */
#define ADDER_VIZ_PLAYER_NO_BAD_EVENT UINT64_MAX

enum { ADDER_VIZ_FRAME_POPPED = 0, ADDER_VIZ_FRAME_RUNNING = 1 };

typedef struct AdderVizPlayerParams {
    uint32_t abi_version;   /* = ADDER_VIZ_PLAYER_ABI_VERSION */
    uint16_t width, height;
    uint8_t channels;       /* 1 or 3 */
    uint8_t codec_version;  /* AbsoluteT handling needs >= 2, the round-up >= 1 (driver.rs:1001, 1093) */
    uint8_t time_mode;      /* ADDER_TIME_* */
    uint8_t has_buffer_limit; /* 0: None */
    uint32_t buffer_limit;  /* > 0 when has_buffer_limit (adder-viz's default: 60) */
    uint32_t tps, ref_interval, delta_t_max;
    float output_fps;       /* Some(fps): tpf = (tps as f32 / fps) as u32; <= 0: None, tpf = ref_interval */
    uint32_t source_camera; /* SourceCamera discriminant; 0..5 = framed */
    uint32_t ring_frames;   /* pending frames kept on the device; 0 = delta_t_max / tpf + 80 */
    int32_t device_id;
    uint8_t view_mode;      /* ADDER_VIEW_* (adder_framer.h): 0 Intensity, 1 D, 2 DeltaT, 3 SAE */
    uint8_t source_type;    /* 0 U8, 1 U16, 2 U32, 3 U64 (Intensity view) */
    uint16_t reserved0;
    float practical_d_max;  /* D view, computed by the caller as for adder_framer.h */
} AdderVizPlayerParams;

typedef struct AdderVizPlayer AdderVizPlayer;

int adder_viz_player_create(const AdderVizPlayerParams *p, AdderVizPlayer **out);
void adder_viz_player_destroy(AdderVizPlayer *pl);
/* Back to the start of a stream: the state of a fresh context, the buffer limit as it stands. */
int adder_viz_player_reset(AdderVizPlayer *pl);
/* Describes the last failure of `pl` (or of the last failed create when pl is null). */
const char *adder_viz_player_last_error(const AdderVizPlayer *pl);
uint32_t adder_viz_player_tpf(const AdderVizPlayer *pl);
int64_t adder_viz_player_frames_written(const AdderVizPlayer *pl);
/* has = 0: None.  Takes effect at the start of the next call. */
int adder_viz_player_set_buffer_limit(AdderVizPlayer *pl, int has, uint32_t limit);

/* n AdderEvents in stream order (device memory).  The frames popped go to d_frames[0 .. *n_frames) in `form`;
 * frame_cap counts frames.  *bad_index = the index of the bad event within this batch, or
 * ADDER_VIZ_PLAYER_NO_BAD_EVENT.  Waits for `stream`. */
int adder_viz_player_ingest_device(AdderVizPlayer *pl, const AdderEvent *d_events, uint64_t n, int form,
                                   uint8_t *d_frames, uint64_t frame_cap, uint64_t *n_frames, int64_t *pop_index,
                                   uint64_t *bad_index, void *stream);
/* The same for n_records raw wire records (the 9 / 11-byte big-endian body of a .adder file). */
int adder_viz_player_ingest_wire_device(AdderVizPlayer *pl, const uint8_t *d_wire, uint64_t n_records, int form,
                                        uint8_t *d_frames, uint64_t frame_cap, uint64_t *n_frames, int64_t *pop_index,
                                        uint64_t *bad_index, uint64_t *n_consumed, void *stream);
/* The end of the stream (device memory). */
int adder_viz_player_finish_device(AdderVizPlayer *pl, int form, uint8_t *d_frames, uint64_t frame_cap,
                                   uint64_t *n_frames, int64_t *pop_index, void *stream);
/* Host-pointer forms: copy in, run on the device, copy the frames out. */
int adder_viz_player_ingest(AdderVizPlayer *pl, const AdderEvent *events, uint64_t n, int form, uint8_t *frames,
                            uint64_t frame_cap, uint64_t *n_frames, int64_t *pop_index, uint64_t *bad_index);
int adder_viz_player_ingest_wire(AdderVizPlayer *pl, const uint8_t *wire, uint64_t n_records, int form,
                                 uint8_t *frames, uint64_t frame_cap, uint64_t *n_frames, int64_t *pop_index,
                                 uint64_t *bad_index, uint64_t *n_consumed);
int adder_viz_player_finish(AdderVizPlayer *pl, int form, uint8_t *frames, uint64_t frame_cap, uint64_t *n_frames,
                            int64_t *pop_index);
/* The running_frame as it stands (host memory). */
int adder_viz_player_running_frame(AdderVizPlayer *pl, uint8_t *frame);

/* Framer::detect_features.  May be switched between any two calls; every call of it clears the carried last event (a
 * UI update lies between two `consume` calls). */
int adder_viz_player_detect_features(AdderVizPlayer *pl, int on);
/* The features of the last ingest call that was not refused, in stream order (finish and refused calls leave the list
 * as it was; reset empties it); `index` is the global stream index of the event (as in pop_index).  *count exceeding
 * `capacity`: ADDER_E_OUT_CAPACITY, nothing is copied. */
int adder_viz_player_features(AdderVizPlayer *pl, AdderFramerFeature *out, uint64_t capacity, uint64_t *count);
/* One FeatureInterval per frame popped by the last ingest / finish call: end_ts[j] (room for that call's *n_frames) and
 * the {x, y} pairs xy[2 * offsets[j] .. 2 * offsets[j + 1]) (offsets: room for *n_frames + 1).  *n_pairs exceeding
 * xy_capacity: ADDER_E_OUT_CAPACITY, nothing is copied.  A refused call leaves the previous call's intervals. */
int adder_viz_player_frame_features(AdderVizPlayer *pl, uint64_t *end_ts, uint64_t *offsets, uint16_t *xy,
                                    uint64_t xy_capacity, uint64_t *n_pairs);
/* FrameSequence::get_running_intensities: the [height][width][channels] u8 plane.  Zeros at create and reset, changed
 * only by calls made with detection on. */
int adder_viz_player_running_intensities(AdderVizPlayer *pl, uint8_t *out);
int adder_viz_player_running_intensities_device(AdderVizPlayer *pl, uint8_t *d_out, void *stream);

/* Where the schedule meets detection, on the host, for self-tests (the functions the kernels run): pops[k] = the local
 * index of the event after which the k-th frame is popped, non-decreasing.  mark_out[i] = mark[i] unless event i is the
 * first of a period; w_out[i] = w0 + the number of pops before event i. */
int adder_viz_features_host(const int32_t *pops, uint32_t n_pops, uint64_t n, const uint8_t *mark, int32_t w0,
                            uint8_t *mark_out, int32_t *w_out);
/* The hand-out's running-frame rule: some / val are the popped frames [n_pops][units], stamps the sorted cross stamps
 * ((unit << 32) | frame k); `running` is read and left as the context's running frame, frames = the RUNNING form. */
int adder_viz_overlay_host(uint32_t units, uint32_t n_pops, const uint8_t *some, const uint8_t *val,
                           const uint64_t *stamps, uint32_t n_stamps, uint8_t *running, uint8_t *frames);

/* The pop schedule on the host, for self-tests: the arithmetic the schedule kernel runs (coverage counts per row and
 * pending frame, forced events by a search in a row-ordered prefix maximum, the period loop), on one whole stream fed
 * to a fresh context in one call.  Per event i of n: row[i]; the fill range (from[i], to[i]] (from == to: none);
 * L[i] = last_filled after the event, or -1 for an event that is not checked.  `finish` != 0 appends the end of the
 * stream.  pop_index[k] = P of the k-th popped frame, flushed[k] = 1 when finish filled its Nones.  Returns the number
 * of popped frames, or -1 when it exceeds `cap` or an argument is out of range. */
int64_t adder_viz_schedule_host(const int32_t *row, const int32_t *from, const int32_t *to, const int32_t *L,
                                uint64_t n, uint32_t rows, uint32_t row_units, int has_limit, uint32_t limit,
                                int finish, int64_t *pop_index, uint8_t *flushed, uint64_t cap);

#ifdef __cplusplus
}
#endif
#endif /* ADDER_VIZ_PLAYER_H */
