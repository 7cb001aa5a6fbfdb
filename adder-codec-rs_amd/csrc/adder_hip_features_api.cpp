// adder_hip_features_api.cpp -- feature-driven rate control and ROI (video.rs:825-837, 865-1112,
// 1291-1293), its halo exchange between row bands, the running-intensities plane and the live view built on it.
#include <string.h>

#include "adder_hip_ctx.hpp"

// the running-intensities plane with its halo rows, on first use
int alloc_running(AdderHipCtx *c, hipStream_t s) {
    if (c->running) return ADDER_OK;
    const size_t bytes = c->n_pad + 2 * halo_bytes(c);
    HIPCHK(c, dalloc(&c->running_base, bytes));
    HIPCHK(c, hipMemsetAsync(c->running_base, 0, bytes, s));
    c->running = c->running_base + halo_bytes(c);
    return ADDER_OK;
}

// a device copy of the running-intensities plane may still be reading it on the caller's stream
int join_ri_copy(AdderHipCtx *c, hipStream_t s) {
    if (c->ri_copy_pending) {
        HIPCHK(c, hipStreamWaitEvent(s, c->ri_copy_e, 0));
        c->ri_copy_pending = false;
    }
    return ADDER_OK;
}

// adder_hip_reset does not wait for its memsets: host-side readers of the state do
static int settle_reset(AdderHipCtx *c) {
    if (c->reset_pending) {
        HIPCHK(c, hipEventSynchronize(c->reset_e));
        c->reset_pending = false;
    }
    return ADDER_OK;
}

extern "C" int adder_hip_update_detect_features(AdderHipCtx *c, int detect_features, int feature_rate_adjustment) {
    if (!c) return ADDER_E_BAD_PARAMS;
    if (c->pending) return fail(c, ADDER_E_BAD_PARAMS, "a device batch is pending");
    if (detect_features && c->continuous) return fail(c, ADDER_E_BAD_PARAMS, "feature detection: FramePerfect contexts only");
    c->feat_detect = detect_features != 0;
    c->feat_adjust = feature_rate_adjustment != 0;
    return ADDER_OK;
}

extern "C" int adder_hip_set_feature_parameters(AdderHipCtx *c, uint8_t c_thresh_baseline, uint16_t feature_c_radius) {
    if (!c) return ADDER_E_BAD_PARAMS;
    if (c->pending) return fail(c, ADDER_E_BAD_PARAMS, "a device batch is pending");
    c->c_thresh_baseline = c_thresh_baseline;
    c->feature_c_radius = feature_c_radius;
    return ADDER_OK;
}

extern "C" int adder_hip_update_roi(AdderHipCtx *c, int enable, uint16_t x0, uint16_t y0, uint16_t x1, uint16_t y1) {
    if (!c) return ADDER_E_BAD_PARAMS;
    if (c->pending) return fail(c, ADDER_E_BAD_PARAMS, "a device batch is pending");
    if (enable && c->continuous) return fail(c, ADDER_E_BAD_PARAMS, "a region of interest: FramePerfect contexts only");
    c->roi_on = enable != 0;
    c->roi[0] = x0;
    c->roi[1] = y0;
    c->roi[2] = x1;
    c->roi[3] = y1;
    return ADDER_OK;
}

extern "C" int adder_hip_feature_set(AdderHipCtx *c, uint8_t *dst) {
    if (!c || !dst) return ADDER_E_BAD_PARAMS;
    if (c->pending) return fail(c, ADDER_E_BAD_PARAMS, "a device batch is pending");
    const size_t n = (size_t)c->rows * c->p.width;
    if (!c->fset) {
        memset(dst, 0, n);
        return ADDER_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    ADDER_TRY(settle_reset(c));
    HIPCHK(c, hipMemcpy(dst, c->fset, n, hipMemcpyDeviceToHost));
    return ADDER_OK;
}

extern "C" int adder_hip_feature_set_device(AdderHipCtx *c, uint8_t *d_dst, void *stream) {
    if (!c || !d_dst) return ADDER_E_BAD_PARAMS;
    if (c->pending) return fail(c, ADDER_E_BAD_PARAMS, "a device batch is pending");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t n = (size_t)c->rows * c->p.width;
    if (!c->fset) {
        HIPCHK(c, hipMemsetAsync(d_dst, 0, n, s));
        return ADDER_OK;
    }
    if (!c->ri_copy_e) HIPCHK(c, hipEventCreateWithFlags(&c->ri_copy_e, hipEventDisableTiming));
    if (!c->ri_src_e) HIPCHK(c, hipEventCreateWithFlags(&c->ri_src_e, hipEventDisableTiming));
    // behind the host-pointer batches and adder_hip_reset's memsets, which queue on the context's stream (no device
    // batch is pending); the next batch waits for the copy as it does for one of the running-intensities plane
    HIPCHK(c, hipEventRecord(c->ri_src_e, c->stream));
    HIPCHK(c, hipStreamWaitEvent(s, c->ri_src_e, 0));
    if (c->pending_stream && c->pending_stream != c->stream && c->pending_stream != s) {
        HIPCHK(c, hipEventRecord(c->ri_src_e, c->pending_stream));
        HIPCHK(c, hipStreamWaitEvent(s, c->ri_src_e, 0));
    }
    HIPCHK(c, hipMemcpyAsync(d_dst, c->fset, n, hipMemcpyDeviceToDevice, s));
    HIPCHK(c, hipEventRecord(c->ri_copy_e, s));
    c->ri_copy_pending = true;
    return ADDER_OK;
}

extern "C" int adder_hip_c_thresh_plane(AdderHipCtx *c, uint8_t *dst) {
    if (!c || !dst) return ADDER_E_BAD_PARAMS;
    if (c->pending) return fail(c, ADDER_E_BAD_PARAMS, "a device batch is pending");
    if (!c->perpx) {
        memset(dst, c->c_thresh, c->n_units);
        return ADDER_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    ADDER_TRY(settle_reset(c));
    HIPCHK(c, hipMemcpy(dst, c->cth_px, c->n_units, hipMemcpyDeviceToHost));
    return ADDER_OK;
}

extern "C" uint32_t adder_hip_last_new_features(const AdderHipCtx *c) { return c ? c->last_new_features : 0u; }

// what the feature kernels take, for a batch with that description (its counters)
FeatureArgs feature_args(const AdderHipCtx *c, const BatchDesc &desc) {
    FeatureArgs fa{};
    fa.fset = c->fset;
    fa.counters = desc.feat_counters;
    fa.chunk_rows = c->p.chunk_rows;
    fa.detect = c->feat_detect ? 1u : 0u;
    fa.radius = (c->feat_detect && c->feat_adjust) ? c->feature_c_radius : 0u;
    fa.low = std::min<uint32_t>(c->c_thresh_baseline, 2u);
    fa.roi_on = c->roi_on ? 1u : 0u;
    fa.rx0 = c->roi[0];
    fa.ry0 = c->roi[1];
    fa.rx1 = c->roi[2];
    fa.ry1 = c->roi[3];
    fa.plane_h = c->p.height;
    fa.new_xy = nullptr;
    fa.new_cap = 0;
    fa.stamp = c->fstamp;
    fa.stamp_base = (uint32_t)(c->frames_done + 1u);  // (enqueue_frames advances frames_done behind the launches)
    return fa;
}

// ---- feature mode across row bands (SURVEY 8(f)4 "needs a halo exchange between row bands") ----
extern "C" size_t adder_hip_feature_halo_bytes(const AdderHipCtx *c) { return c ? halo_bytes(c) : 0; }

extern "C" int adder_hip_feature_halo_export(AdderHipCtx *c, uint8_t *d_top, uint8_t *d_bottom, void *stream) {
    if (!c) return ADDER_E_BAD_PARAMS;
    if (c->pending) return fail(c, ADDER_E_BAD_PARAMS, "a device batch is pending");
    if (!c->running) return fail(c, ADDER_E_BAD_PARAMS, "no running-intensities plane yet (integrate a frame in feature mode first)");
    if (c->rows < kFeatureHalo) return fail(c, ADDER_E_BAD_PARAMS, "a band in feature mode needs at least %u rows", kFeatureHalo);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    const size_t hb = halo_bytes(c), rowlen = (size_t)c->p.width * c->p.channels;
    if (d_top) HIPCHK(c, hipMemcpyAsync(d_top, c->running, hb, hipMemcpyDeviceToDevice, s));
    if (d_bottom) HIPCHK(c, hipMemcpyAsync(d_bottom, c->running + (size_t)(c->rows - kFeatureHalo) * rowlen, hb, hipMemcpyDeviceToDevice, s));
    return ADDER_OK;
}

extern "C" int adder_hip_feature_halo_import(AdderHipCtx *c, const uint8_t *d_above, const uint8_t *d_below, void *stream) {
    if (!c) return ADDER_E_BAD_PARAMS;
    if (c->pending) return fail(c, ADDER_E_BAD_PARAMS, "a device batch is pending");
    if (!c->running) return fail(c, ADDER_E_BAD_PARAMS, "no running-intensities plane yet (integrate a frame in feature mode first)");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    const size_t hb = halo_bytes(c), rowlen = (size_t)c->p.width * c->p.channels;
    if (d_above) HIPCHK(c, hipMemcpyAsync(c->running_base, d_above, hb, hipMemcpyDeviceToDevice, s));
    if (d_below) HIPCHK(c, hipMemcpyAsync(c->running + (size_t)c->rows * rowlen, d_below, hb, hipMemcpyDeviceToDevice, s));
    return ADDER_OK;
}

extern "C" int adder_hip_feature_detect(AdderHipCtx *c, uint32_t *d_new_xy, uint32_t cap, uint32_t *n_new, void *stream) {
    if (!c) return ADDER_E_BAD_PARAMS;
    if (n_new) *n_new = 0;
    if (c->pending) return fail(c, ADDER_E_BAD_PARAMS, "a device batch is pending");
    if (!c->band_frame_pending) return fail(c, ADDER_E_BAD_PARAMS, "no frame awaits its feature step");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    FeatureArgs fa = feature_args(c, c->own);  // (a band's frame is a batch of the blocking calls: the context's own description)
    fa.new_xy = d_new_xy;
    fa.new_cap = d_new_xy ? cap : 0u;
    HIPCHK(c, adder_launch_features(c->own.d_batch, 0u, &fa, s));
    uint32_t cnt[2] = {0u, 0u};
    HIPCHK(c, hipMemcpyAsync(cnt, c->own.feat_counters, sizeof cnt, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    c->band_frame_pending = false;
    c->last_new_features = cnt[0];
    if (n_new) *n_new = cnt[0];
    if (d_new_xy && cnt[0] > cap) return fail(c, ADDER_E_OUT_CAPACITY, "feature list too small: %u new features", cnt[0]);
    return ADDER_OK;
}

extern "C" int adder_hip_feature_apply(AdderHipCtx *c, const uint32_t *d_xy, uint32_t n, void *stream) {
    if (!c) return ADDER_E_BAD_PARAMS;
    if (c->pending) return fail(c, ADDER_E_BAD_PARAMS, "a device batch is pending");
    if (!d_xy && n) return fail(c, ADDER_E_BAD_PARAMS, "null feature list");
    if (!c->perpx || n == 0) return ADDER_OK;  // no per-unit thresholds to reset (detection without rate adjustment)
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    const FeatureArgs fa = feature_args(c, c->own);  // (a band's frame is a batch of the blocking calls: the context's own description)
    HIPCHK(c, adder_launch_feature_apply(c->own.d_batch, &fa, d_xy, n, s));
    return ADDER_OK;
}

extern "C" int adder_hip_enable_running_intensities(AdderHipCtx *c, int enable) {
    if (!c) return ADDER_E_BAD_PARAMS;
    c->running_enabled = enable != 0;
    return ADDER_OK;
}

extern "C" int adder_hip_running_intensities(AdderHipCtx *c, uint8_t *dst) {
    if (!c || !dst) return ADDER_E_BAD_PARAMS;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (!c->running) {  // never enabled before a batch: the plane is still all zeros
        memset(dst, 0, c->n_units);
        return ADDER_OK;
    }
    ADDER_TRY(settle_reset(c));
    HIPCHK(c, hipMemcpy(dst, c->running, c->n_units, hipMemcpyDeviceToHost));
    return ADDER_OK;
}

extern "C" int adder_hip_running_intensities_device(AdderHipCtx *c, uint8_t *d_dst, void *stream) {
    if (!c || !d_dst) return ADDER_E_BAD_PARAMS;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    if (!c->running) {  // never enabled before a batch: the plane is still all zeros
        HIPCHK(c, hipMemsetAsync(d_dst, 0, c->n_units, s));
        return ADDER_OK;
    }
    if (!c->ri_copy_e) HIPCHK(c, hipEventCreateWithFlags(&c->ri_copy_e, hipEventDisableTiming));
    if (!c->ri_src_e) HIPCHK(c, hipEventCreateWithFlags(&c->ri_src_e, hipEventDisableTiming));
    // behind every batch: the host-pointer forms and adder_hip_reset's memsets queue on the context's stream; a device
    // batch on the caller's stream is the last one (the next needs adder_hip_finish, which waits for it) and may still
    // be in flight
    HIPCHK(c, hipEventRecord(c->ri_src_e, c->stream));
    HIPCHK(c, hipStreamWaitEvent(s, c->ri_src_e, 0));
    if (c->pending_stream && c->pending_stream != c->stream && c->pending_stream != s) {
        HIPCHK(c, hipEventRecord(c->ri_src_e, c->pending_stream));
        HIPCHK(c, hipStreamWaitEvent(s, c->ri_src_e, 0));
    }
    HIPCHK(c, hipMemcpyAsync(d_dst, c->running, c->n_units, hipMemcpyDeviceToDevice, s));
    HIPCHK(c, hipEventRecord(c->ri_copy_e, s));
    c->ri_copy_pending = true;
    return ADDER_OK;
}

// ---- the live view (include/adder_hip.h): what the plane shows, and the plane with the features drawn in ----
extern "C" int adder_hip_set_view_mode(AdderHipCtx *c, uint32_t view_mode, float practical_d_max) {
    if (!c) return ADDER_E_BAD_PARAMS;
    if (view_mode > kViewSae) return fail(c, ADDER_E_BAD_PARAMS, "bad view mode %u (ADDER_VIEW_*: 0 .. 3)", view_mode);
    if (practical_d_max != practical_d_max) return fail(c, ADDER_E_BAD_PARAMS, "practical_d_max is NaN");
    if (c->pending || c->f_submitted != c->f_collected) return fail(c, ADDER_E_BAD_PARAMS, "work is in flight on this context");
    c->view_mode = view_mode;
    c->practical_d_max = practical_d_max > 0.0f ? practical_d_max : 0.0f;
    return ADDER_OK;
}

extern "C" int adder_hip_set_show_features(AdderHipCtx *c, uint32_t mode) {
    if (!c) return ADDER_E_BAD_PARAMS;
    if (mode > 2u) return fail(c, ADDER_E_BAD_PARAMS, "bad ShowFeatureMode %u (0 Off, 1 Instant, 2 Hold)", mode);
    if (mode != 0u && is_band(c))
        return fail(c, ADDER_E_BAD_PARAMS, "a row band cannot show features: a cross reaches two rows into the neighbouring band");
    c->show_features = mode;
    return ADDER_OK;
}

// the display frame into device memory on stream s, behind everything the context has queued (no host synchronisation)
static int display_frame_queue(AdderHipCtx *c, uint8_t *d_dst, hipStream_t s) {
    if (is_band(c))
        return fail(c, ADDER_E_BAD_PARAMS, "a row band has no display frame: a cross reaches two rows into the neighbouring band");
    if (!c->running) return fail(c, ADDER_E_BAD_PARAMS, "the running-intensities plane was never enabled before a batch");
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->ri_copy_e) HIPCHK(c, hipEventCreateWithFlags(&c->ri_copy_e, hipEventDisableTiming));
    if (!c->ri_src_e) HIPCHK(c, hipEventCreateWithFlags(&c->ri_src_e, hipEventDisableTiming));
    if (s != c->stream) {  // (adder_hip_running_intensities_device: host-pointer batches and resets queue on the context's stream)
        HIPCHK(c, hipEventRecord(c->ri_src_e, c->stream));
        HIPCHK(c, hipStreamWaitEvent(s, c->ri_src_e, 0));
    }
    if (c->pending_stream && c->pending_stream != c->stream && c->pending_stream != s) {
        HIPCHK(c, hipEventRecord(c->ri_src_e, c->pending_stream));
        HIPCHK(c, hipStreamWaitEvent(s, c->ri_src_e, 0));
    }
    // video.rs:742-744, 883-887: a clone of the plane; crosses only with feature detection on, and only once a frame
    // has been integrated in feature mode (the membership plane exists; frame stamps start at 1)
    const bool crosses = c->show_features != 0u && c->feat_detect && c->fset && c->fstamp && c->frames_done != 0;
    if (crosses)
        HIPCHK(c, adder_launch_display(c->running, c->fset, c->show_features == 1u ? c->fstamp : nullptr, (uint32_t)c->frames_done,
                                       c->p.width, c->rows, c->p.channels, d_dst, s));
    else
        HIPCHK(c, hipMemcpyAsync(d_dst, c->running, c->n_units, hipMemcpyDeviceToDevice, s));
    HIPCHK(c, hipEventRecord(c->ri_copy_e, s));
    c->ri_copy_pending = true;
    return ADDER_OK;
}

extern "C" int adder_hip_display_frame_device(AdderHipCtx *c, uint8_t *d_dst, void *stream) {
    if (!c) return ADDER_E_BAD_PARAMS;
    if (!d_dst) return fail(c, ADDER_E_BAD_PARAMS, "display frame: null destination");
    return display_frame_queue(c, d_dst, (hipStream_t)stream);
}

extern "C" int adder_hip_display_frame(AdderHipCtx *c, uint8_t *dst) {
    if (!c) return ADDER_E_BAD_PARAMS;
    if (!dst) return fail(c, ADDER_E_BAD_PARAMS, "display frame: null destination");
    if (is_band(c) || !c->running) return display_frame_queue(c, nullptr, nullptr);  // (its refusals)
    HIPCHK(c, hipSetDevice(c->device));
    ADDER_TRY(settle_reset(c));
    void *vp = c->d_display;
    ADDER_TRY(ensure(c, &vp, &c->d_display_cap, c->n_units));
    c->d_display = (uint8_t *)vp;
    int rc = display_frame_queue(c, c->d_display, c->stream);
    if (rc != ADDER_OK) return rc;
    HIPCHK(c, hipMemcpyAsync(dst, c->d_display, c->n_units, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ADDER_OK;
}
