/* adder_davis.h -- C-ABI of the DAVIS -> ADDER transcoder (libadder_hip.so).
 *
 * The reference's Davis source (transcoder/source/davis.rs:233-897) on the device.  Its input is what the EDI
 * reconstructor hands to Davis::consume per packet: a deblurred frame of f64 intensities and, in the raw modes, the
 * DVS events before and after the frame's exposure with its start / end timestamps (microseconds) and the contrast
 * threshold c.  (The .aedat4 reader and the reconstructor are not built.)  The camera state -- last timestamp (i64)
 * and last log intensity (f64) per pixel, 0 and 0.0 at create -- lives in HBM; one push is one consume() with a cached
 * packet:
 *   1. start, end and c are taken from the packet (RawDvs: end = start + 1);
 *   2. raw modes: integrate_dvs_events over the PREVIOUS packet's `after` events (an event passes with t < start and,
 *      except in RawDvs, t > the previous end);
 *   3. integrate_dvs_events over this packet's `before` events (t < start);
 *   4. integrate_frame_gaps: every pixel's last intensity from its last event to the start of the frame;
 *   5. the frame as image_8u = saturate(round_half_even(frame * 255)): raw modes one step per pixel in raster order
 *      over end - start ticks as f32 (RawDvs: zeros, c = 0.15, 0 ticks), Framed one dense frame over ref_time;
 *   6. last ln = ln_1p(frame) (RawDvs: ln_1p(0.5)), raw modes last timestamp = end;
 *   7. the `after` events are kept on the device for the next push.
 * An event that passes makes two sparse steps: the pixel's OLD intensity over the time since its last event
 * (ADDER_SPARSE_INTEGRATE_ONLY), then last ln *= exp(+-c) -- a multiplication, as the reference has it -- and the NEW
 * value as ADDER_SPARSE_TEST_ONLY.  The steps of 2..5 go to the sparse integrator in the reference's order: the four
 * row chunks (y / (height / 4)) one after the other, arrival order inside a chunk; gaps and frame in raster order.
 *
 * The inner context is the mirror's Video: one channel, chunk_rows = height / 4, FramePerfect for Framed and
 * Continuous for the raw modes, AbsoluteT, Collapse, the crf given (or the Video's defaults).
 *
 * Refusals, as this library defines them; each changes nothing (state planes, inner context, held `after` events):
 *   an event of `before` or `after` outside the plane   ADDER_DAVIS_E_BAD_EVENT, *bad_index = its index, `before` first
 *   a frame value that is NaN or <= -1 (Framed, RawDavis) ADDER_E_BAD_PARAMS
 *   out_cap below adder_davis_push_capacity()            ADDER_E_OUT_CAPACITY, *n_out = that capacity
 *   a push or finish after finish                        ADDER_DAVIS_E_ORDER
 *   has_events == 0 in a raw mode                        ADDER_E_BAD_PARAMS (the reconstructor always sends them there)
 * In Framed mode the events of a packet are not looked at (n_before and n_after may be 0). */
#ifndef ADDER_DAVIS_H
#define ADDER_DAVIS_H

#include <stddef.h>
#include <stdint.h>

#include "adder_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ADDER_DAVIS_ABI_VERSION 1u
#define ADDER_DAVIS_E_BAD_EVENT (-22)
#define ADDER_DAVIS_E_ORDER (-23)
#define ADDER_DAVIS_NO_CRF (-1) /* no crf call: the Video's defaults */
#define ADDER_DAVIS_NO_BAD_EVENT UINT64_MAX

/* TranscoderMode (davis.rs:41-50) */
enum { ADDER_DAVIS_FRAMED = 0, ADDER_DAVIS_RAW_DAVIS = 1, ADDER_DAVIS_RAW_DVS = 2 };

typedef struct AdderDavisEvent {
    int64_t t; /* microseconds */
    uint16_t x;
    uint16_t y;
    uint8_t on; /* != 0: on */
    uint8_t pad[3];
} AdderDavisEvent;

typedef struct AdderDavisMeta {
    double c;             /* contrast threshold of the packet's events */
    int64_t img_start_ts; /* start / end of the frame's exposure */
    int64_t img_end_ts;
    uint32_t has_events;  /* the reconstructor's Some((c, before, after, start, end)) */
    uint32_t reserved0;
} AdderDavisMeta;

typedef struct AdderDavisParams {
    uint32_t abi_version; /* = ADDER_DAVIS_ABI_VERSION */
    uint16_t width;
    uint16_t height;      /* a multiple of 4 */
    int32_t mode;         /* ADDER_DAVIS_* */
    uint32_t tps;
    uint32_t ref_time;
    uint32_t delta_t_max; /* >= ref_time */
    int32_t crf;          /* 0..9: Davis::new(..).crf(c); ADDER_DAVIS_NO_CRF: no crf call */
    int32_t device_id;
} AdderDavisParams;

typedef struct AdderDavis AdderDavis;

int adder_davis_create(const AdderDavisParams *p, AdderDavis **out);
void adder_davis_destroy(AdderDavis *dv);
/* Back to the state right after create. */
int adder_davis_reset(AdderDavis *dv);
const char *adder_davis_last_error(const AdderDavis *dv);
/* Events one sparse step (Framed: one pixel of a dense frame) can emit at most. */
uint64_t adder_davis_events_per_step(const AdderDavis *dv);
/* The room a push of n_before events needs now: (2 * (held after events + n_before) + 2 * W * H) * events_per_step
 * (Framed: 2 * W * H * events_per_step). */
uint64_t adder_davis_push_capacity(const AdderDavis *dv, uint64_t n_before);

/* One packet.  d_frame: [h][w] f64; d_before / d_after: n_before / n_after events (all device memory; an empty list may
 * be NULL).  The events go to d_out[0 .. *n_out) in the order the reference feeds its encoder; out_cap counts events.
 * Waits for `stream`.  *bad_index = the index of an event outside the plane (`before` first, `after` following), else
 * ADDER_DAVIS_NO_BAD_EVENT. */
int adder_davis_push_device(AdderDavis *dv, const double *d_frame, const AdderDavisMeta *meta,
                            const AdderDavisEvent *d_before, uint64_t n_before, const AdderDavisEvent *d_after,
                            uint64_t n_after, AdderEvent *d_out, uint64_t out_cap, uint64_t *n_out, uint64_t *bad_index,
                            void *stream);
/* The same with host buffers. */
int adder_davis_push_host(AdderDavis *dv, const double *frame, const AdderDavisMeta *meta, const AdderDavisEvent *before,
                          uint64_t n_before, const AdderDavisEvent *after, uint64_t n_after, AdderEvent *out,
                          uint64_t out_cap, uint64_t *n_out, uint64_t *bad_index);
/* End of input (davis.rs:641-669): W * H ADDER_SPARSE_FLUSH steps in raster order in the raw modes (out_cap at least
 * W * H * events_per_step, else refused with *n_out = that), nothing in Framed.  The held `after` events are dropped.
 * Afterwards only reset is accepted. */
int adder_davis_finish_device(AdderDavis *dv, AdderEvent *d_out, uint64_t out_cap, uint64_t *n_out, void *stream);
int adder_davis_finish_host(AdderDavis *dv, AdderEvent *out, uint64_t out_cap, uint64_t *n_out);

/* How many of the last accepted push's events the frame itself made (step 5): the trailing ones of its output, the
 * events Davis::consume returns. */
uint64_t adder_davis_last_frame_events(const AdderDavis *dv);

/* The camera state per pixel in raster order as the last accepted push left it (W * H values each, host buffers;
 * either may be NULL). */
int adder_davis_pixel_state(AdderDavis *dv, int64_t *last_ts, double *last_ln);
/* The inner context's running-intensities side plane (H * W bytes), host buffer. */
int adder_davis_running_intensities(AdderDavis *dv, uint8_t *dst);

/* The chain alone on the CPU -- the functions the kernels run, no context and no GPU.
 * adder_davis_steps_host: integrate_dvs_events over one list.  An event passes with t < check1 and, by check2_mode,
 * 0: no second check, 1: t > check2 (check_dvs_after), 2: t < check2.  last_ts / last_ln: W * H values each, updated in
 * place; steps receives the sparse steps in step order, *n_steps their number.  Refused with nothing changed:
 * ADDER_E_BAD_PARAMS (a null plane, height not a multiple of 4, ref_time 0, a bad check2_mode), ADDER_DAVIS_E_BAD_EVENT
 * (*bad_index = the first event outside the plane), ADDER_E_OUT_CAPACITY (steps_cap < 2 * n; *n_steps = 2 * n). */
int adder_davis_steps_host(uint16_t width, uint16_t height, int64_t *last_ts, double *last_ln, const AdderDavisEvent *events,
                           uint64_t n, int64_t check1, int32_t check2_mode, int64_t check2, double c, uint32_t tps,
                           uint32_t ref_time, AdderSparseStep *steps, uint64_t steps_cap, uint64_t *n_steps,
                           uint64_t *bad_index);
/* integrate_frame_gaps in raster order; steps_cap at least W * H. */
int adder_davis_gaps_host(uint16_t width, uint16_t height, const int64_t *last_ts, double *last_ln, int64_t start,
                          uint32_t tps, uint32_t ref_time, AdderSparseStep *steps, uint64_t steps_cap, uint64_t *n_steps);
/* Steps 5 and 6 of a push: image_8u (W * H bytes, may be NULL), in the raw modes the frame's W * H steps (steps may be
 * NULL in Framed), last ln, and in the raw modes last ts = end.  Refused with nothing changed: a frame value that is NaN
 * or <= -1 in Framed and RawDavis (ADDER_E_BAD_PARAMS). */
int adder_davis_frame_host(uint16_t width, uint16_t height, int32_t mode, const double *frame, int64_t start, int64_t end,
                           int64_t *last_ts, double *last_ln, uint8_t *image_8u, AdderSparseStep *steps);

#ifdef __cplusplus
}
#endif
#endif /* ADDER_DAVIS_H */
