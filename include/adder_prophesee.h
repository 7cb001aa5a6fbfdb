/* adder_prophesee.h -- C-ABI of the Prophesee .dat -> ADDER transcoder (libadder_hip.so).
 *
 * The reference's prophesee_to_adder (transcoder/source/prophesee.rs) on the device.  A .dat recording is a text
 * header of '%' lines, two type bytes, then 8-byte records {u32 t, i32 data} (little-endian).  Every record moves its
 * pixel's log intensity by +-0.02 and becomes up to two integrate_for_px steps: the pixel's previous intensity over
 * the time since its last record, then one source tick of the new one.  The steps go to the sparse integrator
 * (adder_hip_integrate_sparse_device) in camera order on a Continuous context: AbsoluteT, Collapse,
 * tps = ref_time * 10^6, delta_t_max = 2 * ref_time, chunk_rows 1, the running-intensities side plane on.
 *
 * Groups.  The reference reads records until one has t > (running_t at the group's start) + 16666 (u32 wrapping),
 * that record included, then integrates the group; running_t is the max of every t read.  At the end of the input
 * the open group is dropped unintegrated (its t still counts) and end_events integrates every pixel up to running_t.
 * A push therefore integrates only complete groups and keeps the open one for the next push, so the output is the
 * same for any split of the record stream.
 *
 * Errors, as this library defines them.  A record outside the plane inside a group that completes: the push changes
 * nothing and returns ADDER_PROPHESEE_E_BAD_RECORD with the record's index in the stream (records since the start).
 * The same record in the dropped last group is never looked at.  A push or finish whose output may not fit is
 * refused before anything changes (ADDER_E_OUT_CAPACITY, *n_out = a capacity that succeeds).  finish fails with
 * ADDER_PROPHESEE_E_END_ASSERT when a pixel's last t equals running_t (the reference's assert in end_events). */
#ifndef ADDER_PROPHESEE_H
#define ADDER_PROPHESEE_H

#include <stddef.h>
#include <stdint.h>

#include "adder_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ADDER_PROPHESEE_ABI_VERSION 1u
#define ADDER_PROPHESEE_E_BAD_RECORD (-17)
#define ADDER_PROPHESEE_E_END_ASSERT (-18)
#define ADDER_PROPHESEE_E_ORDER (-19)       /* push before start, start twice, or anything after finish */
#define ADDER_PROPHESEE_NO_CRF (-1)         /* no crf call: the Video's defaults (what the C++ mirror runs) */
#define ADDER_PROPHESEE_NO_BAD_RECORD UINT64_MAX
#define ADDER_PROPHESEE_VIEW_INTERVAL 16666u /* PROPHESEE_SOURCE_TPS / 60 */

typedef struct AdderPropheseeHeader {
    uint16_t width;        /* Width / Height lines, defaults 100 x 70, cast to u16 */
    uint16_t height;
    uint32_t header_bytes; /* where the records start */
    uint8_t ev_type;       /* 0 or 12 (0 when there is no '%' line and no type bytes) */
    uint8_t ev_size;       /* 8 (0 when there are no type bytes) */
    uint8_t header_lines;  /* '%' lines, saturated at 255 */
    uint8_t reserved0;
} AdderPropheseeHeader;

/* One decoded record: x = data & 0x3FF (10 bits, a reference quirk: x >= 1024 wraps), y = (data & 0xFFFC000) >> 14,
 * p = bit 28. */
typedef struct AdderPropheseeEvent {
    uint32_t t;
    uint16_t x;
    uint16_t y;
    uint8_t p;
    uint8_t pad[3];
} AdderPropheseeEvent;

typedef struct AdderPropheseeParams {
    uint32_t abi_version; /* = ADDER_PROPHESEE_ABI_VERSION */
    uint16_t width;
    uint16_t height;
    uint32_t ref_time;    /* ADDER ticks per source microsecond, >= 1 */
    int32_t crf;          /* 0..9: Prophesee::new(..).crf(c); ADDER_PROPHESEE_NO_CRF: no crf call */
    int32_t device_id;
} AdderPropheseeParams;

typedef struct AdderProphesee AdderProphesee;

/* parse_header (prophesee.rs:367-422) over the first len bytes of a file.  ADDER_OK; ADDER_E_BAD_PARAMS when the
 * reference refuses (a bad ev_type / ev_size, a plane of width or height 0 after the u16 cast, a Height / Width line
 * whose value word is missing or empty); ADDER_E_OUT_CAPACITY when the buffer ends before the header does and
 * len < file_size (call again with more of the file). */
int adder_prophesee_parse_header(const uint8_t *buf, size_t len, uint64_t file_size, AdderPropheseeHeader *out);
/* decode_event (:437-452) for n 8-byte records. */
void adder_prophesee_decode(const uint8_t *records, uint64_t n, AdderPropheseeEvent *out);
/* The group scan of consume() (:142-170) over n records: *group_start_t = running_t at the open group's start,
 * *running_t = the max t read so far; both are updated.  Returns the number of leading records that complete groups
 * (0 when no record closes one); *groups, when given, receives the groups they complete. */
uint64_t adder_prophesee_scan_groups(const uint8_t *records, uint64_t n, uint32_t *group_start_t, uint32_t *running_t,
                                     uint64_t *groups);

int adder_prophesee_create(const AdderPropheseeParams *p, AdderProphesee **out);
void adder_prophesee_destroy(AdderProphesee *pr);
/* Back to the state right after create (the start-up frames are due again). */
int adder_prophesee_reset(AdderProphesee *pr);
const char *adder_prophesee_last_error(const AdderProphesee *pr);
/* Events one sparse step can emit at most (max_depth + 3): a push of n records needs 2 * n times this at most. */
uint64_t adder_prophesee_events_per_step(const AdderProphesee *pr);

/* The two dense start-up frames of 128 over ref_time (:117-133), host buffer.  out_cap must be at least
 * 2 * adder_hip_max_events_per_frame of the inner context (*n_out says how many when it is not). */
int adder_prophesee_start(AdderProphesee *pr, AdderEvent *out, uint64_t out_cap, uint64_t *n_out);

/* Pushes n records (8 bytes each, the body of a .dat file; device memory) and integrates every group they complete,
 * the open group carried over.  The events go to d_out[0 .. *n_out) in step order; out_cap counts events.  Waits for
 * `stream`.  *bad_index = the stream index of a bad record, else ADDER_PROPHESEE_NO_BAD_RECORD. */
int adder_prophesee_push_device(AdderProphesee *pr, const uint8_t *d_records, uint64_t n, AdderEvent *d_out,
                                uint64_t out_cap, uint64_t *n_out, uint64_t *bad_index, void *stream);
/* The same with host records and a host event buffer. */
int adder_prophesee_push_host(AdderProphesee *pr, const uint8_t *records, uint64_t n, AdderEvent *out,
                              uint64_t out_cap, uint64_t *n_out, uint64_t *bad_index);
/* End of input: drops the open group and runs end_events (:325-365) in raster order; W * H steps, so out_cap must be
 * W * H * adder_prophesee_events_per_step (a smaller buffer is refused and the call may be repeated).  Device and
 * host forms.  After it -- done, or refused with ADDER_PROPHESEE_E_END_ASSERT -- only reset is accepted. */
int adder_prophesee_finish_device(AdderProphesee *pr, AdderEvent *d_out, uint64_t out_cap, uint64_t *n_out,
                                  void *stream);
int adder_prophesee_finish_host(AdderProphesee *pr, AdderEvent *out, uint64_t out_cap, uint64_t *n_out);

/* running_t, the open group's start, the records carried in the open group, the records pushed so far. */
int adder_prophesee_state(const AdderProphesee *pr, uint32_t *running_t, uint32_t *group_start_t,
                          uint64_t *open_records, uint64_t *records_pushed);
/* The camera state per pixel in raster order, as committed by the last accepted push: last t and last log intensity
 * (W * H values each, host buffers; either may be NULL). */
int adder_prophesee_pixel_state(AdderProphesee *pr, uint32_t *last_t, double *last_ln);
/* The running-intensities side plane (H * W bytes), host buffer. */
int adder_prophesee_running_intensities(AdderProphesee *pr, uint8_t *dst);

/* The library's binary64 exp (equal to glibc's): one value and n values on the host, n values on the device. */
double adder_prophesee_exp(double x);
void adder_prophesee_exp_host(const double *x, double *y, uint64_t n);
int adder_prophesee_exp_device(const double *d_x, double *d_y, uint64_t n, int device_id);

#ifdef __cplusplus
}
#endif
#endif /* ADDER_PROPHESEE_H */
