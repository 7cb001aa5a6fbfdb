// adder_hip_sparse_api.cpp -- adder_hip_integrate_sparse* of include/adder_hip.h.
#include <string.h>

#include "adder_hip_ctx.hpp"

// ------------------------------------------------------------------------------------------
// Sparse steps of event-camera sources (adder_sparse.hip): integrate_for_px(px, &mut 0, frame_val, intensity,
// time) per step, in the caller's order; all events into one buffer.
// ------------------------------------------------------------------------------------------
static int sparse_prepare(AdderHipCtx *c, size_t n, hipStream_t s) {
    if (!c->continuous) return fail(c, ADDER_E_BAD_PARAMS, "sparse steps need a Mode::Continuous context (pixel_mode)");
    if (n > 0x7fffffffull) return fail(c, ADDER_E_BAD_PARAMS, "too many steps for one call");
    if (!c->sparse_mode) {
        // c_thresh, its counter and running_t advance per integrate call: from here on they differ between pixels
        if (!c->cth_px) {
            HIPCHK(c, dalloc(&c->cth_px, c->n_pad));
            HIPCHK(c, dalloc(&c->cctr_px, c->n_pad));
        }
        if (!c->rt_px) HIPCHK(c, dalloc(&c->rt_px, c->n_pad));
        HIPCHK(c, hipMemsetAsync(c->cth_px, c->c_thresh, c->n_pad, s));
        HIPCHK(c, hipMemsetAsync(c->cctr_px, c->c_counter, c->n_pad, s));
        uint32_t bits;
        memcpy(&bits, &c->running_t, sizeof bits);
        HIPCHK(c, adder_launch_fill_u32(reinterpret_cast<uint32_t *>(c->rt_px), c->n_pad, bits, s));
        c->sparse_mode = true;
    }
    AdderHipCtx::SparseWork &w = c->sw;
    if (w.cap < n) {
        for (void *p : {(void *)w.steps, (void *)w.keys0, (void *)w.keys1, (void *)w.idx0, (void *)w.idx1, (void *)w.count,
                        (void *)w.offs, (void *)w.stage, w.temp})
            if (p) HIPCHK(c, hipFree(p));
        w = AdderHipCtx::SparseWork{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, w.total, 0, 0};
        const size_t cap = std::max<size_t>(n, 4096);
        HIPCHK(c, dalloc(&w.steps, cap));
        HIPCHK(c, dalloc(&w.keys0, cap));
        HIPCHK(c, dalloc(&w.keys1, cap));
        HIPCHK(c, dalloc(&w.idx0, cap));
        HIPCHK(c, dalloc(&w.idx1, cap));
        HIPCHK(c, dalloc(&w.count, cap));
        HIPCHK(c, dalloc(&w.offs, cap));
        HIPCHK(c, dalloc(&w.stage, cap * (c->max_depth + 3u)));
        w.temp_bytes = adder_sparse_temp_bytes((uint32_t)cap);
        HIPCHK(c, hipMalloc(&w.temp, w.temp_bytes));
        w.cap = cap;
    }
    if (!w.total) HIPCHK(c, dalloc(&w.total, 1));
    return ADDER_OK;
}

static SparseArgs sparse_args(AdderHipCtx *c) {
    SparseArgs a{};
    a.hdr = c->hdr;
    a.lastf = c->lastf;
    a.cn_integ = c->cn_integ;
    a.cn_dt = c->cn_dt;
    a.cn_bdt = c->cn_bdt;
    a.cn_meta = c->cn_meta;
    a.plane_stride = c->n_pad;
    a.cth_px = c->cth_px;
    a.cctr_px = c->cctr_px;
    a.rt_px = c->rt_px;
    a.running = c->running_enabled ? c->running : nullptr;
    a.status = c->status;
    a.c_max = c->p.c_thresh_max;
    a.c_vel = c->p.c_increase_velocity;
    a.max_nodes = c->max_depth + 1u;
    a.stage_events = c->max_depth + 3u;
    a.width = c->p.width;
    a.channels = c->p.channels;
    a.row_begin = c->p.row_begin;
    a.rows = c->rows;
    a.sc = make_consts(c, 0.0f);
    a.view = make_view(c);
    if (!a.running) a.view.view_mode = kViewIntensity;
    return a;
}

// d_steps / d_out: device memory; synchronises `stream` to hand back the count
extern "C" int adder_hip_integrate_sparse_device(AdderHipCtx *c, const AdderSparseStep *d_steps, size_t n, AdderEvent *d_out,
                                                 size_t out_cap, size_t *n_out, void *stream) {
    if (!c) return ADDER_E_BAD_PARAMS;
    if (n_out) *n_out = 0;
    if (c->poisoned) return refuse_poisoned(c);
    if (c->pending || c->f_submitted != c->f_collected) return fail(c, ADDER_E_BAD_PARAMS, "work is in flight on this context");
    if ((!d_steps && n) || (!d_out && out_cap)) return fail(c, ADDER_E_BAD_PARAMS, "null pointer");
    if (n == 0) return ADDER_OK;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if (c->reset_pending) {
        HIPCHK(c, hipStreamWaitEvent(s, c->reset_e, 0));
        c->reset_pending = false;
    }
    ADDER_TRY(join_ri_copy(c, s));
    int rc = sparse_prepare(c, n, s);
    if (rc != ADDER_OK) return rc;
    if (c->running_enabled && !c->running) ADDER_TRY(alloc_running(c, s));
    const SparseArgs a = sparse_args(c);
    AdderHipCtx::SparseWork &w = c->sw;
    HIPCHK(c, adder_sparse_run(&a, reinterpret_cast<const SparseStep *>(d_steps), (uint32_t)n, w.keys0, w.keys1, w.idx0, w.idx1,
                               w.temp, w.temp_bytes, w.stage, w.count, w.offs, reinterpret_cast<AdderEventPod *>(d_out),
                               out_cap, w.total, s));
    unsigned long long total = 0;
    uint32_t st = 0;
    HIPCHK(c, hipMemcpyAsync(&total, w.total, sizeof total, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(&st, c->status, sizeof st, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (n_out) *n_out = (size_t)total;
    c->frames_done += 1;
    if (st & kStatusCapacity) {
        c->poisoned = true;  // the pixels have been stepped: there is no undo on this route
        return fail(c, ADDER_E_OUT_CAPACITY, "event buffer too small: the steps produced %llu events (a buffer of "
                    "n * (max_depth + 3) events cannot overflow)", total);
    }
    return status_to_code(c, st);
}

extern "C" int adder_hip_integrate_sparse(AdderHipCtx *c, const AdderSparseStep *steps, size_t n, AdderEvent *out,
                                          size_t out_cap, size_t *n_out) {
    if (!c) return ADDER_E_BAD_PARAMS;
    if (n_out) *n_out = 0;
    if (!steps && n) return fail(c, ADDER_E_BAD_PARAMS, "steps is null");
    if (!out && out_cap) return fail(c, ADDER_E_BAD_PARAMS, "out is null");
    if (c->poisoned) return refuse_poisoned(c);
    if (c->pending || c->f_submitted != c->f_collected || c->submitted != c->collected)
        return fail(c, ADDER_E_BAD_PARAMS, "work is in flight on this context");
    if (n == 0) return ADDER_OK;
    HIPCHK(c, hipSetDevice(c->device));
    if (c->reset_pending) {
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->reset_e, 0));
        c->reset_pending = false;
    }
    int rc = sparse_prepare(c, n, c->stream);
    if (rc != ADDER_OK) return rc;
    void *vp = c->d_events;
    if ((rc = ensure(c, &vp, &c->d_events_cap, std::max<size_t>(out_cap, 1) * sizeof(AdderEvent))) != ADDER_OK) return rc;
    c->d_events = (AdderEvent *)vp;
    HIPCHK(c, hipMemcpyAsync(c->sw.steps, steps, n * sizeof(SparseStep), hipMemcpyHostToDevice, c->stream));
    size_t total = 0;
    rc = adder_hip_integrate_sparse_device(c, reinterpret_cast<const AdderSparseStep *>(c->sw.steps), n, c->d_events, out_cap,
                                           &total, c->stream);
    if (n_out) *n_out = total;
    if (rc != ADDER_OK) return rc;
    if (total && out) HIPCHK(c, hipMemcpy(out, c->d_events, total * sizeof(AdderEvent), hipMemcpyDeviceToHost));
    return ADDER_OK;
}
