/* adder_stream.h -- C-ABI of the two stream tools of the reference on the device (libadder_hip.so):
 *
 *   migration  adder-codec-rs/src/utils/stream_migration.rs::migrate_v2 and the binary migrate_raw_v0_v1_to_v2:
 *              a DeltaT stream rewritten as an AbsoluteT stream, and its inverse (ours);
 *   info       adder-info/src/main.rs: the report of a stream's header and, with -d, the realised dynamic range,
 *              a fold over every event.
 *
 * Both need every event's time relative to the previous event OF THE SAME UNIT (pixel x channel) in stream order.
 * The library sorts a batch by unit (stable radix sort), works on each unit's run and writes the result back at the
 * event's input index.  The per-unit state persists across calls, so a stream split into batches in any
 * way gives the same bytes and the same (min, max) as one call.
 *
 * MIGRATION.  The direction follows from the two time modes of the parameters:
 *   DeltaT -> AbsoluteT  (forward; migrate_v2 restated).  Per unit a time T, zero at the start.  For each event in
 *       stream order: T += event.t; event.t = T; then, when the INPUT codec version is > 0, the source camera is one
 *       of the six framed ones and T % ref_interval > 0: T = (T / ref_interval + 1) * ref_interval.  D_EMPTY events
 *       are not special: they add their t like any other.  (A Collapse-mode transcoder gives a D_EMPTY event the same
 *       t in both time modes, so migrate_v2 runs ahead of a natively AbsoluteT stream after the first one; that is a
 *       property of the reference's function and is kept.)
 *   AbsoluteT -> DeltaT  (inverse; ours, the exact inverse of the above).  Per unit L, zero at the start:
 *       dt = event.t - L; L = event.t, rounded up to the next multiple of ref_interval when the camera is framed and
 *       event.t % ref_interval != 0.
 *   anything else (equal modes, Mixed on either side): events pass through unchanged and no state moves, which is
 *       what migrate_v2 does with an output mode other than AbsoluteT.
 *   x, y, c, d pass through; a migrated stream has exactly as many events as its input, so d_out == d_in is allowed.
 *   An output record is the WHOLE input record with the four bytes of its time replaced (pass-through: not even
 *   those), out of place as in place: an AdderEvent's pad, and in an 11-byte record with c = None (tag byte 0: d at
 *   byte 5, t at bytes 6..9) the unused byte 10, are the input's.
 *   T is kept in 64 bits, so the round-up itself never overflows; the NEXT event of that unit is the bad one.
 *
 * INFO.  adder_stream_info_* fold a batch into the handle's (min, max) exactly as main.rs:74-121 does event by event
 * (order dependent).  In AbsoluteT streams of codec version >= 2 the event's time is first made
 * relative to the unit's previous RAW time -- no round-up here, as the reference has it.
 *
 * ERRORS, as this library defines them (the reference panics in a debug build and wraps in a release build):
 * forward, T + event.t above UINT32_MAX; inverse and AbsoluteT info, event.t below the unit's previous time; any
 * event outside the plane.  A call that meets one commits the events before it exactly as if the batch had ended
 * there, returns ADDER_STREAM_E_BAD_EVENT with the event's index in *bad_index and applies nothing after it (output
 * records from that index on are not written).  In the wire forms an EOF record (x == y == 0xFFFF) or an
 * undecodable one ends the stream: *n_consumed = the records before it; nothing after it is looked at. */
#ifndef ADDER_STREAM_H
#define ADDER_STREAM_H

#include <stddef.h>
#include <stdint.h>

#include "adder_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ADDER_STREAM_ABI_VERSION 1u
#define ADDER_STREAM_E_BAD_EVENT (-20)
#define ADDER_STREAM_NO_BAD_EVENT UINT64_MAX

typedef struct AdderStreamParams {
    uint32_t abi_version;  /* = ADDER_STREAM_ABI_VERSION */
    uint16_t width;
    uint16_t height;
    uint8_t channels;      /* 1 or 3 */
    uint8_t codec_version; /* of the INPUT stream, 0..3 */
    uint8_t time_mode;     /* of the INPUT stream (ADDER_TIME_*); a v0 / v1 stream is DeltaT */
    uint8_t out_time_mode; /* of the migrated stream; ignored by info */
    uint32_t ref_interval; /* ticks per input frame, > 0 */
    uint32_t source_camera; /* SourceCamera index: 0..5 are framed */
    uint32_t tps;          /* report only */
    uint32_t delta_t_max;  /* report only */
    int32_t device_id;
} AdderStreamParams;

typedef struct AdderStream AdderStream;

/* Fills `p` (out_time_mode = time_mode, device 0) from the header of a raw .adder stream of codec version 0..3.
 * *header_bytes = where the events start, *event_bytes = 9 (one channel) or 11.  ADDER_E_BAD_PARAMS if the buffer
 * (len bytes) is not such a header -- a compressed stream included. */
int adder_stream_parse_header(const uint8_t *buf, size_t len, AdderStreamParams *p, uint32_t *header_bytes,
                              uint32_t *event_bytes);
/* The header of the migrated stream: the input's with time_mode set and the codec version raised to 2 where it was
 * below (a v0 / v1 header has no time-mode field; a v0 header has no source-camera field either and gets FramedU8),
 * everything else byte for byte.  Returns its length (0: not a header) and writes it when it fits in cap bytes.
 * The stream ends with adder_raw_eof's record (adder_hip.h). */
size_t adder_stream_migrated_header(const uint8_t *in_header, size_t len, uint32_t time_mode, uint8_t *out,
                                    size_t cap);

/* ADDER_E_BAD_PARAMS (before any device is touched) for parameters out of range, among them a plane whose
 * width * height * channels + 1 -- the units and the key that sorts bad and EOF records behind them -- does not fit
 * in 32 bits (65535 x 65535 x 3 is such a plane; every one-channel plane fits). */
int adder_stream_create(const AdderStreamParams *p, AdderStream **out);
void adder_stream_destroy(AdderStream *s);
/* Forgets every unit's time (migration and info) and the (min, max) of the fold. */
int adder_stream_reset(AdderStream *s);
/* Describes the last failure of `s` (or of the last failed create when s is null). */
const char *adder_stream_last_error(const AdderStream *s);

/* Migrates n AdderEvents (device, stream order) into d_out[0 .. n) (d_out == d_in allowed).  *bad_index = the index
 * of the bad event within this batch, or ADDER_STREAM_NO_BAD_EVENT.  Waits for `stream`. */
int adder_stream_migrate_device(AdderStream *s, const AdderEvent *d_in, uint64_t n, AdderEvent *d_out,
                                uint64_t *bad_index, void *stream);
/* The same for n_records raw wire records (the 9 / 11-byte big-endian body of a .adder file) into wire records of
 * the same size. */
int adder_stream_migrate_wire_device(AdderStream *s, const uint8_t *d_wire, uint64_t n_records, uint8_t *d_out,
                                     uint64_t *bad_index, uint64_t *n_consumed, void *stream);
/* Host-pointer forms: copy in, migrate on the device, copy the records before the bad / EOF index out. */
int adder_stream_migrate_host(AdderStream *s, const AdderEvent *in, uint64_t n, AdderEvent *out, uint64_t *bad_index);
int adder_stream_migrate_wire_host(AdderStream *s, const uint8_t *wire, uint64_t n_records, uint8_t *out,
                                   uint64_t *bad_index, uint64_t *n_consumed);

/* Folds n events into the handle's (min, max, event count).  Waits for `stream`. */
int adder_stream_info_device(AdderStream *s, const AdderEvent *d_events, uint64_t n, uint64_t *bad_index,
                             void *stream);
int adder_stream_info_wire_device(AdderStream *s, const uint8_t *d_wire, uint64_t n_records, uint64_t *bad_index,
                                  uint64_t *n_consumed, void *stream);
int adder_stream_info_host(AdderStream *s, const AdderEvent *events, uint64_t n, uint64_t *bad_index);
int adder_stream_info_wire_host(AdderStream *s, const uint8_t *wire, uint64_t n_records, uint64_t *bad_index,
                                uint64_t *n_consumed);
/* The fold so far: min_intensity (DBL_MAX before any event), max_intensity, and the events folded. */
int adder_stream_info_range(const AdderStream *s, double *min_intensity, double *max_intensity, uint64_t *n_events);

/* Host helper: adder-info's report (main.rs:47-66, and :137-147 when dynamic_range != 0) for a stream with these
 * parameters, line for line, with the event count given by the caller and without the progress line.  Numbers are
 * Rust's {:.4} ("inf", "-inf", "NaN").  A v0 / v1 stream reads "Time mode: AbsoluteT" as it does there (the
 * reference's decoder keeps its default where the header has no such field).  Returns the text's length; writes it (no terminator) when it fits. */
size_t adder_stream_format_report(const AdderStreamParams *p, uint32_t header_bytes, uint64_t file_bytes,
                                  uint64_t n_events, int dynamic_range, double min_intensity, double max_intensity,
                                  char *out, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* ADDER_STREAM_H */
