/* adder_dvs.h -- C-ABI of the ADDER -> DVS event conversion (libadder_hip.so).
 *
 * The read-side tool of the reference (adder-to-dvs/src/main.rs) on the device: every ADDER event of a unit
 * (pixel x channel) is turned into the log intensity ln_1p(2^d / dt * ref / 255) and compared with the unit's last
 * fired intensity; a change beyond theta / 2 (or the two special windows of main.rs:303-332) fires ONE DVS event
 * {t = the unit's previous time + 1, x, y, polarity}.  Units are independent, a unit's events form a serial chain:
 * the library sorts a batch by unit, evaluates every logarithm in parallel, walks each unit's run with integer time
 * and comparisons only, and scatters the fired events in input order.
 *
 * The per-unit state persists across calls, so a stream converts in batches of any split with the same result as
 * in one call.  ln_1p is a binary64 restatement of the platform libm's (glibc) log1p, bit for bit, host and device.
 *
 * Errors, as this library defines them (the reference stops at the first one): an event of a unit with no state
 * yet whose d > 128, any event with d in 129..=254, any event outside the plane.  A call that meets one commits
 * the events before it exactly as if the batch had ended there, returns ADDER_DVS_E_BAD_EVENT with the event's
 * index in *bad_index and applies nothing after it.  A call whose output does not fit returns ADDER_E_OUT_CAPACITY
 * with the required count in *n_out and changes nothing: call again with a larger buffer. */
#ifndef ADDER_DVS_H
#define ADDER_DVS_H

#include <stddef.h>
#include <stdint.h>

#include "adder_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ADDER_DVS_ABI_VERSION 1u
#define ADDER_DVS_E_BAD_EVENT (-16)
#define ADDER_DVS_NO_BAD_EVENT UINT64_MAX

/* Output record formats */
enum { ADDER_DVS_OUT_EVENTS = 0, /* AdderDvsEvent, 16 bytes */
       ADDER_DVS_OUT_DAT = 1 };  /* Prophesee .dat record, 8 bytes: u32 t (LE), u32 p << 28 | y << 14 | x (LE) */

typedef struct AdderDvsEvent {
    uint64_t t; /* the full time (text output); the .dat record keeps its low 32 bits */
    uint16_t x;
    uint16_t y;
    uint8_t p; /* 1 = positive, 0 = negative */
    uint8_t pad[3];
} AdderDvsEvent;

typedef struct AdderDvsParams {
    uint32_t abi_version; /* = ADDER_DVS_ABI_VERSION */
    uint16_t width;
    uint16_t height;
    uint8_t channels;      /* 1 or 3 */
    uint8_t time_mode;     /* ADDER_TIME_DELTA_T (0) or anything else (AbsoluteT rules) */
    uint16_t reserved0;
    uint32_t ref_interval; /* ticks per input frame (meta.ref_interval) */
    uint32_t source_camera; /* SourceCamera index: 0..5 are framed (time rounded up to ref_interval) */
    double theta;          /* DVS contrast threshold (CLI default 0.01) */
    int32_t device_id;
} AdderDvsParams;

typedef struct AdderDvs AdderDvs;

/* Fills `p` (theta = 0.01, device 0) from the header of a raw .adder stream of codec version 0..3.
 * *header_bytes = where the events start, *event_bytes = 9 (one channel) or 11.  ADDER_E_BAD_PARAMS if the buffer
 * (len bytes) is not such a header. */
int adder_dvs_parse_header(const uint8_t *buf, size_t len, AdderDvsParams *p, uint32_t *header_bytes,
                           uint32_t *event_bytes);

int adder_dvs_create(const AdderDvsParams *p, AdderDvs **out);
void adder_dvs_destroy(AdderDvs *dvs);
/* Forgets every unit's state (the next event of each unit is its first again). */
int adder_dvs_reset(AdderDvs *dvs);
/* Describes the last failure of `dvs` (or of the last failed create when dvs is null). */
const char *adder_dvs_last_error(const AdderDvs *dvs);

/* Converts n AdderEvents (device, stream order) and appends nothing: the fired DVS events of this batch are written
 * to d_out[0 .. *n_out) in `out_format`, in input order.  out_cap counts records.  *bad_index = the index of the bad
 * event within this batch, or ADDER_DVS_NO_BAD_EVENT.  Waits for `stream` (the counts are needed on the host). */
int adder_dvs_convert_device(AdderDvs *dvs, const AdderEvent *d_events, uint64_t n, int out_format, void *d_out,
                             uint64_t out_cap, uint64_t *n_out, uint64_t *bad_index, void *stream);
/* The same for n_records raw wire records on the device (the 9 / 11-byte big-endian body of a .adder file).  An EOF
 * record (x == y == 0xFFFF) or an undecodable one ends the stream: *n_consumed = the records before it (n_records
 * when there is none).  Records after it are not looked at. */
int adder_dvs_convert_wire_device(AdderDvs *dvs, const uint8_t *d_wire, uint64_t n_records, int out_format,
                                  void *d_out, uint64_t out_cap, uint64_t *n_out, uint64_t *bad_index,
                                  uint64_t *n_consumed, void *stream);
/* Host-pointer forms of the two: copy in, convert on the device, copy the records out. */
int adder_dvs_convert_host(AdderDvs *dvs, const AdderEvent *events, uint64_t n, int out_format, void *out,
                           uint64_t out_cap, uint64_t *n_out, uint64_t *bad_index);
int adder_dvs_convert_wire_host(AdderDvs *dvs, const uint8_t *wire, uint64_t n_records, int out_format, void *out,
                                uint64_t out_cap, uint64_t *n_out, uint64_t *bad_index, uint64_t *n_consumed);

/* --reorder: a stable sort of n output records (device, `out_format`) by their 32-bit time (the low word of an
 * AdderDvsEvent's t); equal times keep their order.  The caller keeps the whole output and sorts once at the end. */
int adder_dvs_sort_device(AdderDvs *dvs, void *d_records, uint64_t n, int out_format, void *stream);

/* ---- The DVS event video and the event-count map (main.rs:189-239, 288, 382-411, 424-448).  Off by default. ----
 *
 * The reference keeps a deque of gray frames [frame_count, end): before each ADDER event, when
 * current_t > frame_count * L + B, it pops (writes) the front frame and frame_count advances -- also when the deque
 * is empty, so those indices are skipped.  L = (tps as f32 / fps) as u128 ticks per frame, B = (tps as f32 *
 * buffer_secs) as u128.  A fired DVS event {old_t + 1, x, y, p} belongs to frame (old_t + 1) / L: it sets pixel
 * (y, x) to 255 (p = 1) or 0 (p = 0) on a 128 background, the deque growing to reach it, unless that frame was
 * already popped (then the event is dropped from the video only).  The reference never joins its drawing call to its
 * fire points; the join here is that of its sibling tool (bin_cv/aedat4_dvs_visualize.rs:132-145, 203-206), and
 * draw = 0 gives the reference's literal output, blank frames.  Built here: the frames as [h][w] u8 planes (the
 * reference's frame is that plane three times) with their frame indices, and the per-unit event-count map.  Not
 * built: the mp4 encoder, the on-screen display, a viewer for plain .dat recordings.
 *
 * Pending frames live in a ring of ring_frames planes on the device, and so do the frames a call emitted until they
 * are popped.  A convert call that needs more slots than the ring has returns ADDER_E_OUT_CAPACITY and changes
 * nothing, like one whose DVS output does not fit; adder_dvs_video_ring_needed tells the slots it asked for. */
typedef struct AdderDvsVideoParams {
    uint32_t abi_version; /* = ADDER_DVS_ABI_VERSION */
    uint32_t tps;         /* ticks per second (meta.tps) */
    float fps;            /* finite, > 0, and tps / fps >= 1 (CLI default 100) */
    float buffer_secs;    /* CLI default 10; negative and NaN count as 0 */
    uint32_t ring_frames; /* 0: ceil(B / L) + 64 */
    uint32_t draw;        /* 1: fired events are drawn; 0: the reference's literal blank frames */
} AdderDvsVideoParams;

/* Fills tps from the header of a raw .adder stream and the CLI's defaults: fps 100, buffer_secs 10, draw 1,
 * ring_frames 0. */
int adder_dvs_video_params_from_header(const uint8_t *buf, size_t len, AdderDvsVideoParams *p);
/* Enables the video and the count map.  Only on a context that converted no event since its create or last reset
 * (adder_dvs_reset also puts the video back to its start).  ADDER_E_BAD_PARAMS: fps not finite or not positive, L = 0. */
int adder_dvs_video_enable(AdderDvs *dvs, const AdderDvsVideoParams *p);
/* The frames emitted by the convert calls (and the finish) since the last pop. */
int adder_dvs_video_frames_ready(AdderDvs *dvs, uint64_t *n);
/* Ring slots the last convert or finish call needed (at most ring_frames unless it failed for them). */
int adder_dvs_video_ring_needed(AdderDvs *dvs, uint64_t *n);
/* Hands the ready frames out, oldest first, as [*n_popped][h][w] bytes to `d_out` (device) / `out` (host), and their
 * frame indices to frame_index (a host array of out_cap_frames entries in both forms, may be null).  More ready frames
 * than out_cap_frames: ADDER_E_OUT_CAPACITY with their number in *n_popped, nothing changes. */
int adder_dvs_video_pop_device(AdderDvs *dvs, uint8_t *d_out, uint64_t out_cap_frames, uint64_t *frame_index,
                               uint64_t *n_popped, void *stream);
int adder_dvs_video_pop(AdderDvs *dvs, uint8_t *out, uint64_t out_cap_frames, uint64_t *frame_index,
                        uint64_t *n_popped);
/* The stream's end: the final check, then every pending frame (one blank frame when there is none) becomes ready.
 * After a bad event this check is the one the reference makes in front of the event that fails: the stream ends there.
 * Convert calls are refused afterwards, until a reset. */
int adder_dvs_video_finish(AdderDvs *dvs);
/* The event-count map, [h][w][3] bytes: 128 everywhere, and for c < channels
 * ((count as u16) as f32 / m as f32 * 255.0) as u8 with m = min(largest count of a unit, 65535). */
int adder_dvs_event_count_map_device(AdderDvs *dvs, uint8_t *d_out, void *stream);
int adder_dvs_event_count_map(AdderDvs *dvs, uint8_t *out);
/* ---- For self-tests only (as adder_dvs_log1p below): the video's arithmetic on the host, without a device.  A program
 * that converts streams needs none of the five. ---- */
/* What adder_dvs_video_enable asks of `p`, without a context: ADDER_OK or ADDER_E_BAD_PARAMS; *L and *B (may be null)
 * receive the frame length and the buffer in ticks. */
int adder_dvs_video_params_check(const AdderDvsVideoParams *p, uint64_t *L, uint64_t *B);
/* L, B, and one byte of the count map. */
uint64_t adder_dvs_video_frame_length(uint32_t tps, float fps);
uint64_t adder_dvs_video_buffer_ticks(uint32_t tps, float buffer_secs);
uint8_t adder_dvs_video_count_byte(uint32_t count, uint32_t m);
/* The schedule of one call as the kernels compute it (adder_dvs_video_logic.hpp): pt[i] = the unit's time after
 * event i (0: a first event), fire_t[i] = old_t + 1 of a fired event (0: none), state = {frame_count, current_t, end},
 * in and out.  Returns the number of emitted frames; pop / accept (n marks each) and emitted (cap indices) may be
 * null. */
uint64_t adder_dvs_video_schedule_host(const uint64_t *pt, const uint64_t *fire_t, uint64_t n, uint64_t L, uint64_t B,
                                       int draw, uint64_t *state, uint8_t *pop, uint8_t *accept, uint64_t *emitted,
                                       uint64_t cap);

/* Host helpers.  The .dat / text header: "% Height h\n% Width w\n% Version 2\n% Date <date>\n% end\n", and in binary
 * mode the two bytes 00 08.  Returns the header's length; writes it when it fits in cap bytes. */
size_t adder_dvs_header_bytes(uint16_t width, uint16_t height, const char *date, int binary, char *out, size_t cap);
/* One text line "t x y p\n" per event; returns the bytes the lines take, writes them when they fit in cap. */
size_t adder_dvs_format_text(const AdderDvsEvent *events, uint64_t n, char *out, size_t cap);
/* The library's binary64 log1p (the one the kernels use), on the host: one value, and n values of an array. */
double adder_dvs_log1p(double x);
void adder_dvs_log1p_host(const double *x, double *y, uint64_t n);
/* Evaluates the same routine on the device for n inputs (device pointers), for self-tests. */
int adder_dvs_log1p_device(const double *d_x, double *d_y, uint64_t n, int device_id);

#ifdef __cplusplus
}
#endif
#endif /* ADDER_DVS_H */
