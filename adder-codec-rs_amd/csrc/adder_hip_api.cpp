// adder_hip_api.cpp -- C-ABI of the MI355X framed->ADDER integration path (include/adder_hip.h).
//
// Owns what Video<W> owns for this path in the reference (video.rs:322-346): the pixel
// state (here: structure-of-arrays planes in HBM) and the step parameters; the caller
// owns frames and event buffers.  There is NO CPU fallback: without a gfx950 device
// adder_hip_create fails with ADDER_E_NO_DEVICE.
//
// This file: the context's life, its settings, the integrate_* entry points and adder_hip_finish, and the host-buffer
// forms.  The other roles of the ABI are in the files adder_hip_ctx.hpp lists.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <new>

#include "adder_color_kernels.h"
#include "adder_hip_ctx.hpp"

static_assert(sizeof(AdderEvent) == 12, "AdderEvent must be 12 bytes");
static_assert(sizeof(AdderEventPod) == sizeof(AdderEvent), "layout mismatch");

static thread_local std::string g_create_error;

int fail(AdderHipCtx *ctx, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx)
        ctx->err = buf;
    else
        g_create_error = buf;
    return code;
}

int refuse_poisoned(AdderHipCtx *c) {
    return fail(c, ADDER_E_POISONED, "context is poisoned by an earlier failure: %s", c->err.c_str());
}

static void free_ctx(AdderHipCtx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    void *ptrs[] = {c->state_slab, c->dv_integ, c->dv_dt,
                    c->dv_bdt,  c->dv_bd,   c->running_base, c->d_new_xy, c->cn_integ, c->cn_dt, c->cn_bdt, c->cn_meta,
                    c->snap.cn_integ, c->snap.cn_dt, c->snap.cn_bdt, c->snap.cn_meta,
                    c->d_offsets, c->d_frames, c->d_rgb, c->d_events, c->d_chunks, c->d_wire,
                    c->cth_px, c->cctr_px, c->fset, c->fstamp, c->d_display, c->own.feat_counters, c->snap.cth_px, c->snap.cctr_px, c->snap.fset,
                    c->snap.fstamp,
                    c->snap.running};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    for (void *p : {(void *)c->park_ring, (void *)c->wtot_ring, (void *)c->wpref_ring, (void *)c->ftot_ring,
                    (void *)c->wofs_ring, (void *)c->wcur})
        if (p) (void)hipFree(p);
    for (auto &sl : c->slot) {
        if (sl.d_wire) (void)hipFree(sl.d_wire);
        if (sl.h_wire) (void)hipHostFree(sl.h_wire);
        if (sl.h_offsets) (void)hipHostFree(sl.h_offsets);
        if (sl.done) (void)hipEventDestroy(sl.done);
        if (sl.wired) (void)hipEventDestroy(sl.wired);
    }
    for (auto &fs : c->fslot) {
        if (fs.out_graph) (void)hipGraphExecDestroy(fs.out_graph);
        for (void *p : {(void *)fs.d_frame, (void *)fs.d_rgb, (void *)fs.d_events, (void *)fs.d_offsets, (void *)fs.desc.d_batch,
                        (void *)fs.desc.feat_counters})
            if (p) (void)hipFree(p);
        for (void *p : {(void *)fs.h_events, (void *)fs.h_hdr, (void *)fs.desc.h_batch})
            if (p) (void)hipHostFree(p);
        if (fs.done) (void)hipEventDestroy(fs.done);
    }
    if (c->frame_e) (void)hipEventDestroy(c->frame_e);
    if (c->out_s) (void)hipStreamDestroy(c->out_s);
    if (c->in_s) (void)hipStreamDestroy(c->in_s);
    for (hipStream_t d : c->ring_streams) (void)hipStreamDestroy(d);
    if (c->in_e) (void)hipEventDestroy(c->in_e);
    for (void *p : {(void *)c->snap.slab, (void *)c->snap.dv_integ, (void *)c->snap.dv_dt, (void *)c->snap.dv_bdt,
                    (void *)c->snap.dv_bd})
        if (p) (void)hipFree(p);
    for (hipEvent_t e : c->launch_events) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->post_events) (void)hipEventDestroy(e);
    if (c->d_rec_total) (void)hipFree(c->d_rec_total);
    if (c->d_side_words) (void)hipFree(c->d_side_words);
    if (c->d_rr_tab) (void)hipFree(c->d_rr_tab);
    if (c->d_lr_tab) (void)hipFree(c->d_lr_tab);
    if (c->d_band_desc) (void)hipFree(c->d_band_desc);
    if (c->h_band_desc) (void)hipHostFree(c->h_band_desc);
    for (hipEvent_t e : c->band_desc_e)
        if (e) (void)hipEventDestroy(e);
    if (c->d_timeline) (void)hipFree(c->d_timeline);
    for (void *p : {(void *)c->rt_px, (void *)c->sw.steps, (void *)c->sw.keys0, (void *)c->sw.keys1, (void *)c->sw.idx0,
                    (void *)c->sw.idx1, (void *)c->sw.count, (void *)c->sw.offs, (void *)c->sw.stage, c->sw.temp,
                    (void *)c->sw.total})
        if (p) (void)hipFree(p);
    for (auto &kv : c->graphs.keys)
        for (GraphHandle e : kv.second.cand)
            if (e) (void)hipGraphExecDestroy(static_cast<hipGraphExec_t>(e));
    for (GraphHandle e : c->retired_execs) (void)hipGraphExecDestroy(static_cast<hipGraphExec_t>(e));
    if (c->own.d_batch) (void)hipFree(c->own.d_batch);  // (a description's blocks start at its BatchArgs)
    if (c->own.h_batch) (void)hipHostFree(c->own.h_batch);
    if (c->h_result) (void)hipHostFree(c->h_result);
    if (c->reset_e) (void)hipEventDestroy(c->reset_e);
    if (c->ri_copy_e) (void)hipEventDestroy(c->ri_copy_e);
    if (c->ri_src_e) (void)hipEventDestroy(c->ri_src_e);
    for (hipEvent_t e : {c->cap_e1, c->cap_e2[0], c->cap_e2[1], c->cap_e2[2], c->cap_e2[3], c->cap_e2[4]})
        if (e) (void)hipEventDestroy(e);
    if (c->cap_s) (void)hipStreamDestroy(c->cap_s);
    if (c->cap_s2) (void)hipStreamDestroy(c->cap_s2);
    if (c->null_join) (void)hipEventDestroy(c->null_join);
    if (c->ev_start) (void)hipEventDestroy(c->ev_start);
    if (c->ev_stop) (void)hipEventDestroy(c->ev_stop);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

extern "C" void adder_hip_default_params(AdderHipParams *p, uint16_t width, uint16_t height, uint8_t channels) {
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->abi_version = ADDER_HIP_ABI_VERSION;
    p->width = width;
    p->height = height;
    p->channels = channels;
    p->time_mode = ADDER_TIME_ABSOLUTE_T;   // TimeMode::default (lib.rs:77-79)
    p->multi_mode = ADDER_MULTI_COLLAPSE;   // PixelMultiMode::default (lib.rs:211-212)
    p->pixel_mode = ADDER_MODE_FRAME_PERFECT;
    p->row_begin = 0;
    p->row_end = height;
    p->ref_time = 255;      // VideoStateParams::default (video.rs:173-182)
    p->delta_t_max = 7650;
    p->c_thresh_max = 7;    // Crf::new(None) -> quality 3 (rate_controller.rs:21,55-70)
    p->c_increase_velocity = 7;
    p->c_thresh_start = 10; // PixelArena::new (event_pixel_tree.rs:82-83)
    p->c_counter_start = 1;
    p->chunk_rows = 1;      // VideoState::default (video.rs:230)
    p->max_depth = 16;
    p->device_id = -1;
}

// Video::new (video.rs:350-438): every pixel = PixelArena::new(1.0, coord): base_val 0,
// c_thresh 10, counter 1, one pristine node (m = 0), last_fired_t 0, running_t 0.
static int init_state(AdderHipCtx *c) {
    const AdderHipParams &p = c->p;
    // header word 0 = base_val 0, no fired level, not popped.  The level planes are only read where
    // the header says they are live (or are selected away: lean step), so they need no clearing.
    if (c->continuous) {
        // PixelArena::new(1.0): one node {d: 0, integration 0, delta_t 0, no best event}, length 1
        const size_t cnt = c->n_pad * (c->max_depth + 1u);
        HIPCHK(c, adder_launch_fill_u32(c->hdr, c->n_pad, apx_hdr(APx{0u, 1u, false, 0.0f}), c->stream));
        HIPCHK(c, hipMemsetAsync(c->cn_integ, 0, cnt * sizeof(float), c->stream));
        HIPCHK(c, hipMemsetAsync(c->cn_dt, 0, cnt * sizeof(float), c->stream));
        HIPCHK(c, hipMemsetAsync(c->cn_bdt, 0, cnt * sizeof(float), c->stream));
        HIPCHK(c, hipMemsetAsync(c->cn_meta, 0, cnt * sizeof(uint32_t), c->stream));
        HIPCHK(c, hipMemsetAsync(c->lastf, 0, c->n_pad * sizeof(float), c->stream));
        HIPCHK(c, hipMemsetAsync(c->status, 0, kStatusBlockBytes, c->stream));
    } else {
        HIPCHK(c, hipMemsetAsync(c->state_slab, 0, c->reset_bytes, c->stream));  // hdr, last_fired_t, status, d_run_max
    }
    if (c->running_base) HIPCHK(c, hipMemsetAsync(c->running_base, 0, c->n_pad + 2 * halo_bytes(c), c->stream));
    c->band_frame_pending = false;
    c->c_thresh = p.c_thresh_start;
    c->c_counter = p.c_counter_start;
    c->generic_sticky = false;
    c->frac_time_seen = false;
    c->cr_valid = true;
    c->cr_time = 0.0f;
    c->run_bound = 0;
    c->pending_reports = false;
    c->dtm_max_seen = p.delta_t_max;
    c->perpx = false;
    c->sparse_mode = false;
    if (c->fset) HIPCHK(c, hipMemsetAsync(c->fset, 0, (size_t)c->rows * p.width, c->stream));
    if (c->fstamp) HIPCHK(c, hipMemsetAsync(c->fstamp, 0, (size_t)c->rows * p.width * sizeof(uint32_t), c->stream));
    c->running_t = 0.0f;
    c->frames_done = 0;
    c->poisoned = false;
    return ADDER_OK;
}

extern "C" int adder_hip_create(const AdderHipParams *params, AdderHipCtx **out) {
    if (!out) return fail(nullptr, ADDER_E_BAD_PARAMS, "out is null");
    *out = nullptr;
    if (!params) return fail(nullptr, ADDER_E_BAD_PARAMS, "params is null");
    AdderHipParams p = *params;
    if (p.abi_version != ADDER_HIP_ABI_VERSION)
        return fail(nullptr, ADDER_E_BAD_PARAMS, "abi_version %u != %u", p.abi_version, ADDER_HIP_ABI_VERSION);
    if (p.width == 0 || p.height == 0)  // PlaneSize::new (lib.rs:103-118)
        return fail(nullptr, ADDER_E_BAD_PARAMS, "invalid plane %ux%ux%u", p.width, p.height, p.channels);
    if (p.channels != 1 && p.channels != 3)
        return fail(nullptr, ADDER_E_BAD_PARAMS, "channels must be 1 or 3 (got %u)", p.channels);
    if (p.pixel_mode != ADDER_MODE_FRAME_PERFECT && p.pixel_mode != ADDER_MODE_CONTINUOUS)
        return fail(nullptr, ADDER_E_BAD_PARAMS, "bad pixel_mode");
    if (p.time_mode > ADDER_TIME_MIXED || p.multi_mode > ADDER_MULTI_COLLAPSE)
        return fail(nullptr, ADDER_E_BAD_PARAMS, "bad time_mode / multi_mode");
    if (p.row_begin == 0 && p.row_end == 0) p.row_end = p.height;
    if (p.row_begin >= p.row_end || p.row_end > p.height)
        return fail(nullptr, ADDER_E_BAD_PARAMS, "bad row band [%u,%u) of %u", p.row_begin, p.row_end, p.height);
    if (p.ref_time == 0) return fail(nullptr, ADDER_E_BAD_PARAMS, "ref_time must be > 0");
    if (p.delta_t_max < p.ref_time)  // video.rs:527-533
        return fail(nullptr, ADDER_E_BAD_PARAMS, "delta_t_max %u is smaller than ref_time %u", p.delta_t_max,
                    p.ref_time);
    if (p.delta_t_max % p.ref_time != 0)  // framed.rs:100-109
        return fail(nullptr, ADDER_E_BAD_PARAMS, "delta_t_max must be a multiple of ref_time");
    if (p.c_increase_velocity == 0) return fail(nullptr, ADDER_E_BAD_PARAMS, "c_increase_velocity must be >= 1");
    if (p.chunk_rows == 0) p.chunk_rows = 1;
    if (p.max_depth == 0) p.max_depth = 16;
    if (p.max_depth > kMaxDepthLimit)
        return fail(nullptr, ADDER_E_BAD_PARAMS, "max_depth must be <= %u", kMaxDepthLimit);

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, ADDER_E_NO_DEVICE, "no HIP device visible; this path has no CPU fallback");
    int dev = p.device_id;
    if (dev < 0) {
        if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    }
    if (dev >= ndev) return fail(nullptr, ADDER_E_BAD_PARAMS, "device_id %d out of range (%d devices)", dev, ndev);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess)
        return fail(nullptr, ADDER_E_HIP, "hipGetDeviceProperties failed");
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, ADDER_E_NO_DEVICE, "device %d is %s; this library is built for gfx950 only", dev,
                    prop.gcnArchName);

    AdderHipCtx *c = new (std::nothrow) AdderHipCtx();
    if (!c) return fail(nullptr, ADDER_E_HIP, "out of host memory");
    c->p = p;
    c->device = dev;
    c->num_cus = (uint32_t)prop.multiProcessorCount;
    c->rows = p.row_end - p.row_begin;
    const uint64_t units = (uint64_t)c->rows * p.width * p.channels;
    // the kernels address a state plane with 32-bit byte offsets: 4 bytes per unit below 4 GiB
    if (units > 0x3ffffc00ull) {
        delete c;
        return fail(nullptr, ADDER_E_BAD_PARAMS, "row band too large (%llu pixel-channels)", (unsigned long long)units);
    }
    c->n_units = (uint32_t)units;
    // pad to a whole number of K1 blocks and of segment groups (the expand kernel's unit)
    {
        const uint32_t quantum = std::max<uint32_t>(kTileUnits, (uint32_t)ADDER_EXPAND_SEGS * kWaveUnits);
        c->n_pad = (size_t)((c->n_units + quantum - 1) / quantum) * quantum;
        c->num_tiles = (uint32_t)(c->n_pad / kTileUnits);  // K1 blocks
    }
    c->num_waves = (uint32_t)(c->n_pad / kWaveUnits);
    c->num_chunks = (c->rows + p.chunk_rows - 1) / p.chunk_rows;
    c->max_depth = p.max_depth;
    // Crf::new(None, plane): quality 3 -> feature_c_radius = (CRF[3][3] * min_resolution as f32) as u16
    // (rate_controller.rs:17,66-67)
    c->feature_c_radius = (uint16_t)((1.0f / 15.0f) * (float)std::min<uint32_t>(p.width, p.height));

    int rc = ADDER_OK;
    auto setup = [&]() -> int {
        HIPCHK(c, hipSetDevice(dev));
        HIPCHK(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        HIPCHK(c, hipEventCreate(&c->ev_start));
        HIPCHK(c, hipEventCreate(&c->ev_stop));
        {
            // The five level-0 planes come from one allocation, each pushed a few KiB further than the one before:
            // separate allocations of this size all start on the same 2 MiB boundary, a wave then reads the same
            // offset of four planes at once, and whether those four streams fall on the same HBM channels was left
            // to the allocator (measured: the same build ran at 1.82 or 1.97 ms per step from context to context).
            const size_t skew = 4352;
            const size_t plane = (c->n_pad * sizeof(uint32_t) + 255) & ~(size_t)255;
            c->slab_bytes = 5 * (plane + skew) + kStatusBlockBytes;
            HIPCHK(c, dalloc(&c->state_slab, c->slab_bytes));
            // header plane, last_fired_t plane and the status block first: what a reset clears is one range.  The block
            // holds every word a reset zeroes: the status word and, a cache line on, the integer-state kernels' run report
            // (adder_publish_kernel clears that one behind every batch as well)
            uint8_t *q = c->state_slab;
            c->hdr = reinterpret_cast<uint32_t *>(q);
            c->lastf = reinterpret_cast<float *>(q + 1 * (plane + skew));
            c->status = reinterpret_cast<uint32_t *>(q + 2 * (plane + skew));
            c->d_run_max = c->status + 32;
            c->reset_bytes = 2 * (plane + skew) + kStatusBlockBytes;
            q += kStatusBlockBytes;
            c->integ0 = reinterpret_cast<float *>(q + 2 * (plane + skew));
            c->dt0 = reinterpret_cast<float *>(q + 3 * (plane + skew));
            c->bdt0 = reinterpret_cast<float *>(q + 4 * (plane + skew));
        }
        c->continuous = p.pixel_mode == ADDER_MODE_CONTINUOUS;
        if (c->continuous) {
            const size_t cnt = c->n_pad * (c->max_depth + 1u);
            HIPCHK(c, dalloc(&c->cn_integ, cnt));
            HIPCHK(c, dalloc(&c->cn_dt, cnt));
            HIPCHK(c, dalloc(&c->cn_bdt, cnt));
            HIPCHK(c, dalloc(&c->cn_meta, cnt));
        }
        ADDER_TRY(alloc_scratch(c, c->continuous ? kScratchCont
                                   : p.time_mode == ADDER_TIME_ABSOLUTE_T ? kScratchLean : kScratchLean8));
        ADDER_TRY(alloc_batch_desc(c, &c->own, 1024));
        HIPCHK(c, hipHostMalloc(reinterpret_cast<void **>(&c->h_result), sizeof(BatchResult), hipHostMallocDefault));
        memset(c->h_result, 0, sizeof(BatchResult));
        HIPCHK(c, hipEventCreateWithFlags(&c->reset_e, hipEventDisableTiming));
        HIPCHK(c, hipStreamCreateWithFlags(&c->cap_s, hipStreamNonBlocking));
        {
            // scan / offsets / expansion of chunk k share the chip with the frame kernel of chunk k+1: the short
            // scan must not queue behind a grid that fills every CU, or the expansion starts a whole kernel late
            int lo_prio = 0, hi_prio = 0;
            HIPCHK(c, hipDeviceGetStreamPriorityRange(&lo_prio, &hi_prio));
            HIPCHK(c, hipStreamCreateWithPriority(&c->cap_s2, hipStreamNonBlocking, hi_prio));
        }
        HIPCHK(c, hipEventCreateWithFlags(&c->cap_e1, hipEventDisableTiming));
        for (hipEvent_t &e : c->cap_e2) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        if (const char *ng = getenv("ADDER_HIP_NO_GRAPH")) {
            c->use_graph = atoi(ng) == 0;
            c->eager_two_streams = atoi(ng) == 2;
        }
        {
            // workgroups per CU of the lean frame kernel and of the expansion when they share the chip (0: full grids)
            const char *lb = getenv("ADDER_HIP_LEAN_BLOCKS_PER_CU"), *eb = getenv("ADDER_HIP_EXPAND_BLOCKS_PER_CU");
            // (full grids since the frame kernel runs 5 waves per SIMD and the streams carry cache hints: walking
            // grids of 4 + 3 workgroups per CU, the default until then, measured 2-3 % slower)
            c->lean_blocks_per_cu = lb ? (uint32_t)atoi(lb) : 0u;
            c->expand_blocks_per_cu = eb ? (uint32_t)atoi(eb) : 0u;
        }
        if (const char *gc = getenv("ADDER_HIP_GRAPH_CANDIDATES")) c->graph_candidates = (uint32_t)std::max(1, atoi(gc));
        if (const char *fl = getenv("ADDER_HIP_FRAMES_PER_LAUNCH"))
            c->frames_per_launch = (uint32_t)std::max(1, std::min<int>(atoi(fl), kMaxFramesPerLaunch));
        HIPCHK(c, dalloc(&c->d_rec_total, 1));
        HIPCHK(c, dalloc(&c->d_side_words, 4));  // ([2]: a constant 0 -- the wire scatter's destination of a lone frame)
        HIPCHK(c, hipMemsetAsync(c->d_side_words, 0, 4 * sizeof(uint64_t), c->stream));
        HIPCHK(c, dalloc(&c->d_chunks, c->num_chunks + 1));
        ADDER_TRY(init_state(c));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return ADDER_OK;
    };
    rc = setup();
    if (rc != ADDER_OK) {
        g_create_error = c->err;
        free_ctx(c);
        return rc;
    }
    *out = c;
    return ADDER_OK;
}

extern "C" void adder_hip_destroy(AdderHipCtx *ctx) { free_ctx(ctx); }

extern "C" const char *adder_hip_last_error(const AdderHipCtx *ctx) {
    return ctx ? ctx->err.c_str() : g_create_error.c_str();
}

extern "C" int adder_hip_set_crf_parameters(AdderHipCtx *c, uint8_t c_thresh_max, uint8_t c_increase_velocity) {
    if (!c) return ADDER_E_BAD_PARAMS;
    if (c_increase_velocity == 0) return fail(c, ADDER_E_BAD_PARAMS, "c_increase_velocity must be >= 1");
    c->p.c_thresh_max = c_thresh_max;
    c->p.c_increase_velocity = c_increase_velocity;
    return ADDER_OK;
}

extern "C" int adder_hip_reset_c_thresh(AdderHipCtx *c, uint8_t baseline) {
    if (!c) return ADDER_E_BAD_PARAMS;
    if (c->pending || c->f_submitted != c->f_collected || c->submitted != c->collected)
        return fail(c, ADDER_E_BAD_PARAMS, "work is in flight on this context (finish / collect it first)");
    // every pixel: c_thresh = baseline, c_increase_counter = 0 (video.rs:1247-1250,1283-1286); the pair
    // is uniform across the plane, so it lives in the context
    c->c_thresh = baseline;
    c->c_counter = 0;
    c->perpx = false;  // uniform again; the next frame of a feature / ROI batch re-creates the planes from the pair
    if (c->sparse_mode && c->cth_px) {  // sparse contexts keep the pair per unit: every unit gets (baseline, 0)
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, hipMemsetAsync(c->cth_px, baseline, c->n_pad, c->stream));
        HIPCHK(c, hipMemsetAsync(c->cctr_px, 0, c->n_pad, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return ADDER_OK;
}

extern "C" int adder_hip_set_delta_t_max(AdderHipCtx *c, uint32_t dtm) {
    if (!c) return ADDER_E_BAD_PARAMS;
    if (dtm < c->p.ref_time || dtm % c->p.ref_time != 0)
        return fail(c, ADDER_E_BAD_PARAMS, "delta_t_max must be a multiple of ref_time and >= ref_time");
    c->p.delta_t_max = dtm;
    c->dtm_max_seen = std::max(c->dtm_max_seen, dtm);
    return ADDER_OK;
}

extern "C" int adder_hip_set_time_mode(AdderHipCtx *c, uint8_t time_mode) {
    if (!c) return ADDER_E_BAD_PARAMS;
    if (time_mode > ADDER_TIME_MIXED) return fail(c, ADDER_E_BAD_PARAMS, "bad time_mode");
    if (c->frames_done != 0)
        return fail(c, ADDER_E_BAD_PARAMS, "time mode can only be set before the first frame is integrated");
    c->p.time_mode = time_mode;
    return ADDER_OK;
}

extern "C" uint32_t adder_hip_num_chunks(const AdderHipCtx *c) { return c ? c->num_chunks : 0; }

extern "C" size_t adder_hip_max_events_per_frame(const AdderHipCtx *c) {
    return c ? worst_case_events_per_frame(c, (float)c->p.ref_time) : 0;
}

int status_to_code(AdderHipCtx *c, uint32_t st) {
    if (st == 0) return ADDER_OK;
    c->poisoned = true;
    if (st & kStatusDepth)
        return fail(c, ADDER_E_ARENA_DEPTH, "a pixel needed more than max_depth=%u stored nodes", c->max_depth);
    if (st & kStatusWire)
        return fail(c, ADDER_E_BAD_PARAMS, "wire serialisation: an event without a channel on a multi-channel plane");
    if (st & kStatusSparse) return fail(c, ADDER_E_BAD_PARAMS, "a sparse step names a pixel outside the plane / row band");
    if (st & kStatusScratch) return fail(c, ADDER_E_HIP, "internal error: a segment's record log exceeded its bound");
    if (st & kStatusLeanRuns)
        return fail(c, ADDER_E_HIP, "internal error: the lean-runs kernel met state planes outside its regime (popped_dtm != (base_val != 0))");
    return fail(c, ADDER_E_OUT_CAPACITY, "event buffer too small");
}

// a row band in feature / ROI mode: refused before anything is queued (a caller's mistake, not a poisoned context)
static int band_precheck(AdderHipCtx *c, uint32_t num_frames) {
    if (!band_features(c)) return ADDER_OK;
    if (num_frames > 1)
        return fail(c, ADDER_E_BAD_PARAMS, "a row band in feature / ROI mode integrates one frame per call (the halo "
                    "exchange and adder_hip_feature_detect come between the frames)");
    if (c->band_frame_pending)
        return fail(c, ADDER_E_BAD_PARAMS, "the previous frame's feature step is missing (adder_hip_feature_detect)");
    return ADDER_OK;
}

// stream == NULL means "the default stream" to a caller, and the context's own stream is a non-blocking one: whatever the
// caller queued on the legacy default stream -- a torch.zeros() of the offsets, the clip's generator -- is NOT ordered against
// it.  (Round 5's "a 3-frame batch left its offsets untouched" was this: the test's zero-fill of the offsets tensor, on the
// null stream, landing AFTER the short batch had written them; tests/test_gpu_stress.py holds the arrangement.)  So a batch
// submitted with stream == NULL first waits for the default stream's work queued so far.
int join_null_stream(AdderHipCtx *c) {
    static const bool off = env_flag("ADDER_HIP_DBG_NO_NULL_JOIN");  // (tests/test_gpu_stress.py shows the race with it)
    if (off) return ADDER_OK;
    if (!c->null_join) HIPCHK(c, hipEventCreateWithFlags(&c->null_join, hipEventDisableTiming));
    HIPCHK(c, hipEventRecord(c->null_join, nullptr));
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->null_join, 0));
    return ADDER_OK;
}

// the *_rgb entry points exist for one-channel contexts only (a colour context takes the colour frame as it is)
int rgb_precheck(AdderHipCtx *c) {
    if (c->p.channels != 1)
        return fail(c, ADDER_E_BAD_PARAMS, "colour frames are converted for a channels == 1 context only (this one has %u "
                    "channels and takes them as they are)", c->p.channels);
    return ADDER_OK;
}

// A device batch into AdderEvents, or (wire) into the raw sink's records: d_out then holds bytes, out_cap counts records.
// rgb: d_frames holds [num_frames][rows][width][3]; the batch reads their gray form (adder_color.hip) out of c->d_frames.
// The conversion goes on the batch's stream in front of it -- behind the NULL-stream join, outside the captured graphs --
// and c->d_frames is not written again before the batch has been finished: the next batch is refused until then.
static int integrate_device(AdderHipCtx *c, const uint8_t *d_frames, uint32_t num_frames, float time_spanned, AdderEvent *d_out,
                            size_t out_cap, uint64_t *d_frame_offsets, void *stream, bool wire, bool rgb = false) {
    if (c->poisoned) return refuse_poisoned(c);
    if (c->pending) return fail(c, ADDER_E_BAD_PARAMS, "previous device batch not finished (call adder_hip_finish)");
    if (c->f_submitted != c->f_collected)
        return fail(c, ADDER_E_BAD_PARAMS, "frames are in flight (call adder_hip_frame_collect)");
    if (!d_frames || !d_frame_offsets || (!d_out && out_cap)) return fail(c, ADDER_E_BAD_PARAMS, "null pointer");
    // AdderEvents leave as dwords (every expansion); wire records are bytes and may start anywhere (include/adder_hip.h)
    if (!wire && ((uintptr_t)d_out & 3u) != 0u)
        return fail(c, ADDER_E_BAD_PARAMS, "d_out must be 4-byte aligned (AdderEvent alignment)");
    if (!(time_spanned >= 0.0f)) return fail(c, ADDER_E_BAD_PARAMS, "time_spanned must be >= 0");
    ADDER_TRY(band_precheck(c, num_frames));
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if (!stream) ADDER_TRY(join_null_stream(c));
    if (rgb && num_frames != 0) {
        void *vp = c->d_frames;
        ADDER_TRY(ensure(c, &vp, &c->d_frames_cap, (size_t)num_frames * c->n_units + 16));
        c->d_frames = (uint8_t *)vp;
        HIPCHK(c, color_to_gray_launch(d_frames, (uint64_t)c->p.width * 3u, (uint64_t)c->n_units * 3u, c->d_frames, c->p.width,
                                       c->n_units, c->p.width, c->rows, num_frames, s));
        d_frames = c->d_frames;
    }
    if (num_frames == 0) {
        HIPCHK(c, hipMemsetAsync(d_frame_offsets, 0, sizeof(uint64_t), s));
    } else {
        BatchRequest rq;
        rq.d_frames = d_frames;
        rq.num_frames = num_frames;
        rq.time_spanned = time_spanned;
        rq.d_out = d_out;
        rq.out_cap = out_cap;
        rq.d_offsets = d_frame_offsets;
        rq.stream = s;
        rq.wire = wire;
        rq.desc = &c->own;
        BatchQueued done;
        int rc = enqueue_frames(c, rq, &done);
        if (rc != ADDER_OK) {
            c->poisoned = true;
            return rc;
        }
    }
    c->pending = true;
    c->pending_stream = s;
    c->pending_offsets = d_frame_offsets;
    c->pending_frames = num_frames;
    c->pending_cap = out_cap;
    return ADDER_OK;
}

extern "C" int adder_hip_integrate_device(AdderHipCtx *c, const uint8_t *d_frames, uint32_t num_frames,
                                          float time_spanned, AdderEvent *d_out, size_t out_cap,
                                          uint64_t *d_frame_offsets, void *stream) {
    if (!c) return ADDER_E_BAD_PARAMS;
    return integrate_device(c, d_frames, num_frames, time_spanned, d_out, out_cap, d_frame_offsets, stream, false);
}

// The same batch with the raw sink's records as its output (include/adder_hip.h)
extern "C" int adder_hip_integrate_wire_device(AdderHipCtx *c, const uint8_t *d_frames, uint32_t num_frames, float time_spanned,
                                               uint8_t *d_wire, size_t wire_cap_bytes, uint64_t *d_frame_offsets, void *stream) {
    if (!c) return ADDER_E_BAD_PARAMS;
    return integrate_device(c, d_frames, num_frames, time_spanned, reinterpret_cast<AdderEvent *>(d_wire),
                            wire_cap_bytes / wire_record_bytes(c), d_frame_offsets, stream, true);
}

extern "C" int adder_hip_integrate_rgb_device(AdderHipCtx *c, const uint8_t *d_rgb_frames, uint32_t num_frames, float time_spanned,
                                              AdderEvent *d_out, size_t out_cap, uint64_t *d_frame_offsets, void *stream) {
    if (!c) return ADDER_E_BAD_PARAMS;
    ADDER_TRY(rgb_precheck(c));
    return integrate_device(c, d_rgb_frames, num_frames, time_spanned, d_out, out_cap, d_frame_offsets, stream, false, true);
}

extern "C" int adder_hip_integrate_wire_rgb_device(AdderHipCtx *c, const uint8_t *d_rgb_frames, uint32_t num_frames,
                                                   float time_spanned, uint8_t *d_wire, size_t wire_cap_bytes,
                                                   uint64_t *d_frame_offsets, void *stream) {
    if (!c) return ADDER_E_BAD_PARAMS;
    ADDER_TRY(rgb_precheck(c));
    return integrate_device(c, d_rgb_frames, num_frames, time_spanned, reinterpret_cast<AdderEvent *>(d_wire),
                            wire_cap_bytes / wire_record_bytes(c), d_frame_offsets, stream, true, true);
}

extern "C" void *adder_hip_last_batch_stream(AdderHipCtx *c) {
    return c ? (void *)(c->pending_stream ? c->pending_stream : c->stream) : nullptr;
}
extern "C" int adder_hip_sync_last_batch_stream(AdderHipCtx *c) {
    if (!c) return ADDER_E_BAD_PARAMS;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->pending_stream ? c->pending_stream : c->stream));
    return ADDER_OK;
}

extern "C" int adder_hip_finish(AdderHipCtx *c, size_t *n_out) {
    if (!c) return ADDER_E_BAD_PARAMS;
    if (!c->pending) return fail(c, ADDER_E_BAD_PARAMS, "no device batch pending");
    c->pending = false;
    HIPCHK(c, hipSetDevice(c->device));
    uint32_t st = 0;
    uint64_t total = 0;
    c->last_new_features = 0;
    if (c->pending_frames && !(c->own.feat_counters && feature_path(c))) {
        // the batch's last node wrote {events, records, status} into page-locked memory: wait for the event behind
        // it, no copies
        // (a short spin on the flag the last node sets: an event wait parks the thread and wakes up tens of
        // microseconds late; the event is behind the flag in the same stream, so the wait below is then immediate)
        {
            volatile uint32_t *flag = &c->h_result->valid;
            const auto t_end = std::chrono::steady_clock::now() + std::chrono::milliseconds(20);
            uint32_t spins = 0;
            while (!*flag && ((++spins & 1023u) != 0u || std::chrono::steady_clock::now() < t_end)) {
            }
        }
        HIPCHK(c, hipEventSynchronize(c->ev_stop));
        if (!c->h_result->valid) return fail(c, ADDER_E_HIP, "the batch finished without publishing its result");
        st = c->h_result->status;
        total = c->h_result->total_events;
        c->last_records = c->h_result->records;
        if (c->pending_reports)  // the longest run at the batch's end (0: below kRunReportMin) + whatever was queued behind it
            c->run_bound = std::min<uint64_t>(c->run_bound, (uint64_t)std::max(c->h_result->max_run, kRunReportMin) +
                                                                (c->frames_done - c->pending_end_frames));
        c->pending_reports = false;
    } else {
        HIPCHK(c, hipMemcpyAsync(&st, c->status, sizeof st, hipMemcpyDeviceToHost, c->pending_stream));
        HIPCHK(c, hipMemcpyAsync(&total, c->pending_offsets + c->pending_frames, sizeof total, hipMemcpyDeviceToHost,
                                 c->pending_stream));
        HIPCHK(c, hipMemcpyAsync(&c->last_records, c->d_rec_total, sizeof(uint64_t), hipMemcpyDeviceToHost,
                                 c->pending_stream));
        if (c->own.feat_counters && feature_path(c))
            HIPCHK(c, hipMemcpyAsync(&c->last_new_features, c->own.feat_counters, sizeof(uint32_t), hipMemcpyDeviceToHost,
                                     c->pending_stream));
        HIPCHK(c, hipStreamSynchronize(c->pending_stream));
    }
    if (c->pending_frames)
        HIPCHK(c, hipEventElapsedTime(&c->last_ms, c->ev_start, c->ev_stop));
    else
        c->last_ms = 0.0f;
    graph_tune_report(c, c->last_ms);
    c->last_launch_avg_us = 0.0f;
    if (c->timed_launches) {
        double sum = 0.0;
        for (uint32_t f = 0; f < c->timed_pairs; ++f) {
            float ms = 0.0f;
            HIPCHK(c, hipEventElapsedTime(&ms, c->launch_events[2 * f], c->launch_events[2 * f + 1]));
            sum += ms;
        }
        c->last_launch_avg_us = (float)(sum * 1000.0 / c->timed_launches);
    }
    c->last_post_avg_us = 0.0f;
    if (c->timed_posts) {
        double sum = 0.0;
        for (uint32_t k = 0; k < c->timed_posts; ++k) {
            float ms = 0.0f;
            HIPCHK(c, hipEventElapsedTime(&ms, c->post_events[2 * k], c->post_events[2 * k + 1]));
            sum += ms;
        }
        c->last_post_avg_us = (float)(sum * 1000.0 / c->timed_posts);
    }
    if (n_out) *n_out = (size_t)total;
    if (st == kStatusCapacity && c->snap.valid) {
        // the event buffer was too small: nothing else went wrong, and the state before the batch is at hand
        int rc = restore_snapshot(c, c->pending_stream);
        c->band_frame_pending = false;  // (the frame is gone with the rollback: the retry is a fresh integrate call)
        if (rc != ADDER_OK) {
            c->poisoned = true;
            return rc;
        }
        return fail(c, ADDER_E_OUT_CAPACITY, "event buffer too small: the batch needs %llu events (state rolled back, "
                    "retry with a larger buffer)", (unsigned long long)total);
    }
    c->snap.valid = false;
    // (a total beyond the caller's buffer with no capacity status cannot come out of a sound batch: refuse it here rather
    // than hand the caller a count it would copy by)
    if (st == 0u && total > (uint64_t)c->pending_cap) {
        c->poisoned = true;
        return fail(c, ADDER_E_HIP, "the batch reports %llu events for a buffer of %llu without a capacity status (frame offsets damaged)",
                    (unsigned long long)total, (unsigned long long)c->pending_cap);
    }
    const int rc_st = status_to_code(c, st);
    if (rc_st != ADDER_OK) c->band_frame_pending = false;  // (no feature step follows a failed frame)
    return rc_st;
}

extern "C" float adder_hip_last_batch_ms(AdderHipCtx *c) { return c ? c->last_ms : 0.0f; }

// diagnostics: the last batch's kernel timeline (ADDER_HIP_TIMELINE=1), [4 kinds][64 chunks][start, end] in 10 ns ticks
extern "C" int adder_hip_debug_timeline(AdderHipCtx *c, unsigned long long *dst) {
    if (!c || !dst || !c->d_timeline) return ADDER_E_BAD_PARAMS;
    HIPCHK(c, hipMemcpy(dst, c->d_timeline, 4 * kTimelineChunks * 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return ADDER_OK;
}

extern "C" unsigned adder_hip_last_batch_kernel(const AdderHipCtx *c) {
    if (!c) return ADDER_KERNEL_LEAN;
    return variant_frame_kernel(c->last_variant);
}

extern "C" int adder_hip_set_launch_timing(AdderHipCtx *c, int enable) {
    if (!c) return ADDER_E_BAD_PARAMS;
    c->launch_timing = enable == 2 ? 2 : (enable != 0 ? 1 : 0);
    return ADDER_OK;
}

extern "C" float adder_hip_last_launch_avg_us(AdderHipCtx *c) { return c ? c->last_launch_avg_us : 0.0f; }

extern "C" float adder_hip_last_post_avg_us(AdderHipCtx *c) { return c ? c->last_post_avg_us : 0.0f; }
extern "C" uint32_t adder_hip_last_post_chunks(AdderHipCtx *c) { return c ? c->timed_posts : 0u; }
extern "C" uint64_t adder_hip_last_batch_records(AdderHipCtx *c) { return c ? c->last_records : 0ull; }
extern "C" uint32_t adder_hip_chunk_frames(const AdderHipCtx *c) { return c ? c->chunk : 0u; }
extern "C" uint32_t adder_hip_segment_units(void) { return kWaveUnits; }
extern "C" uint32_t adder_hip_wire_record_bytes(const AdderHipCtx *c) { return c ? wire_record_bytes(c) : 0u; }

extern "C" float adder_hip_last_launch_frames(AdderHipCtx *c) {
    return (c && c->timed_launches) ? (float)c->timed_frames / (float)c->timed_launches : 0.0f;
}

extern "C" int adder_hip_set_frames_per_launch(AdderHipCtx *c, uint32_t frames) {
    if (!c) return ADDER_E_BAD_PARAMS;
    if (frames < 1 || frames > kMaxFramesPerLaunch)
        return fail(c, ADDER_E_BAD_PARAMS, "frames_per_launch must be in 1..%u", kMaxFramesPerLaunch);
    c->frames_per_launch = frames;
    return ADDER_OK;
}

extern "C" int adder_hip_reset(AdderHipCtx *c) {
    if (!c) return ADDER_E_BAD_PARAMS;
    if (c->pending) return fail(c, ADDER_E_BAD_PARAMS, "a device batch is pending (call adder_hip_finish)");
    if (c->f_submitted != c->f_collected || c->submitted != c->collected)
        return fail(c, ADDER_E_BAD_PARAMS, "frames are in flight (collect them first)");
    HIPCHK(c, hipSetDevice(c->device));
    ADDER_TRY(join_ri_copy(c, c->stream));
    ADDER_TRY(init_state(c));
    // the memsets are queued on the context's stream; whoever touches the state next orders itself behind them
    // (enqueue_frames: a stream wait; the host-side accessors: settle_reset)
    HIPCHK(c, hipEventRecord(c->reset_e, c->stream));
    c->reset_pending = true;
    return ADDER_OK;
}

int ensure(AdderHipCtx *c, void **p, size_t *cap, size_t need) {
    if (*cap >= need && *p) return ADDER_OK;
    if (*p) HIPCHK(c, hipFree(*p));
    *p = nullptr;
    *cap = 0;
    HIPCHK(c, hipMalloc(p, std::max<size_t>(need, 16)));
    *cap = need;
    return ADDER_OK;
}

// Host frames -> device, integrate, finish: the events of the batch end up in c->d_events
// (capacity out_cap events), the frame offsets in c->d_offsets; *total = number of events.
// rgb: the frames are [rows][width][3]; they are uploaded to c->d_rgb and the batch converts them (integrate_device).
int batch_to_device(AdderHipCtx *c, const uint8_t *frames, uint32_t num_frames, size_t frame_stride, size_t row_stride,
                    float time_spanned, size_t out_cap, size_t *total, bool rgb) {
    *total = 0;
    if (c->poisoned) return refuse_poisoned(c);
    if (c->pending) return fail(c, ADDER_E_BAD_PARAMS, "a device batch is pending (call adder_hip_finish)");
    if (!frames && num_frames) return fail(c, ADDER_E_BAD_PARAMS, "frames is null");
    const size_t rowlen = (size_t)c->p.width * (rgb ? 3u : c->p.channels);
    const size_t frame_bytes = rowlen * c->rows;  // (gray: n_units)
    if (row_stride == 0) row_stride = rowlen;
    if (row_stride < rowlen) return fail(c, ADDER_E_BAD_PARAMS, "row_stride_bytes smaller than a row");
    if (frame_stride == 0) frame_stride = row_stride * c->rows;
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    void *vp = rgb ? c->d_rgb : c->d_frames;
    if ((rc = ensure(c, &vp, rgb ? &c->d_rgb_cap : &c->d_frames_cap, (size_t)num_frames * frame_bytes + 16)) != ADDER_OK) return rc;
    (rgb ? c->d_rgb : c->d_frames) = (uint8_t *)vp;
    uint8_t *const d_in = (uint8_t *)vp;
    vp = c->d_events;
    if ((rc = ensure(c, &vp, &c->d_events_cap, out_cap * sizeof(AdderEvent))) != ADDER_OK) return rc;
    c->d_events = (AdderEvent *)vp;
    vp = c->d_offsets;
    if ((rc = ensure(c, &vp, &c->d_offsets_cap, ((size_t)num_frames + 1) * sizeof(uint64_t))) != ADDER_OK) return rc;
    c->d_offsets = (uint64_t *)vp;

    if (row_stride == rowlen && frame_stride == frame_bytes) {  // packed: one linear copy
        HIPCHK(c, hipMemcpyAsync(d_in, frames, (size_t)num_frames * frame_bytes, hipMemcpyHostToDevice, c->stream));
    } else {
        for (uint32_t f = 0; f < num_frames; ++f)
            HIPCHK(c, hipMemcpy2DAsync(d_in + (size_t)f * frame_bytes, rowlen, frames + (size_t)f * frame_stride,
                                       row_stride, rowlen, c->rows, hipMemcpyHostToDevice, c->stream));
    }
    rc = integrate_device(c, d_in, num_frames, time_spanned, c->d_events, out_cap, c->d_offsets, c->stream, false, rgb);
    if (rc != ADDER_OK) return rc;
    rc = adder_hip_finish(c, total);
    if (rc != ADDER_OK) return rc;  // ADDER_E_OUT_CAPACITY: rolled back, *total = the size needed
    return ADDER_OK;
}

static int integrate_batch(AdderHipCtx *c, const uint8_t *frames, uint32_t num_frames, size_t frame_stride, size_t row_stride,
                           float time_spanned, AdderEvent *out, size_t out_cap, size_t *n_out, uint64_t *frame_offsets, bool rgb) {
    if (n_out) *n_out = 0;
    if (rgb) ADDER_TRY(rgb_precheck(c));
    if (!out && out_cap) return fail(c, ADDER_E_BAD_PARAMS, "out is null");
    size_t total = 0;
    int rc = batch_to_device(c, frames, num_frames, frame_stride, row_stride, time_spanned, out_cap, &total, rgb);
    if (n_out) *n_out = total;
    if (rc != ADDER_OK) return rc;
    if (total) HIPCHK(c, hipMemcpy(out, c->d_events, total * sizeof(AdderEvent), hipMemcpyDeviceToHost));
    if (frame_offsets)
        HIPCHK(c, hipMemcpy(frame_offsets, c->d_offsets, ((size_t)num_frames + 1) * sizeof(uint64_t),
                            hipMemcpyDeviceToHost));
    return ADDER_OK;
}

extern "C" int adder_hip_integrate_batch(AdderHipCtx *c, const uint8_t *frames, uint32_t num_frames,
                                         size_t frame_stride, size_t row_stride, float time_spanned,
                                         AdderEvent *out, size_t out_cap, size_t *n_out,
                                         uint64_t *frame_offsets) {
    if (!c) return ADDER_E_BAD_PARAMS;
    return integrate_batch(c, frames, num_frames, frame_stride, row_stride, time_spanned, out, out_cap, n_out, frame_offsets, false);
}

extern "C" int adder_hip_integrate_batch_rgb(AdderHipCtx *c, const uint8_t *frames_hwc3, uint32_t num_frames, size_t frame_stride,
                                             size_t row_stride, float time_spanned, AdderEvent *out, size_t out_cap,
                                             size_t *n_out, uint64_t *frame_offsets) {
    if (!c) return ADDER_E_BAD_PARAMS;
    return integrate_batch(c, frames_hwc3, num_frames, frame_stride, row_stride, time_spanned, out, out_cap, n_out, frame_offsets, true);
}

extern "C" int adder_hip_integrate_batch_raw(AdderHipCtx *c, const uint8_t *frames, uint32_t num_frames,
                                             size_t frame_stride, size_t row_stride, float time_spanned,
                                             uint8_t *out_bytes, size_t out_cap_bytes, size_t *n_bytes,
                                             size_t *n_events, uint64_t *frame_offsets) {
    if (!c) return ADDER_E_BAD_PARAMS;
    if (n_bytes) *n_bytes = 0;
    if (n_events) *n_events = 0;
    if (!out_bytes && out_cap_bytes) return fail(c, ADDER_E_BAD_PARAMS, "out_bytes is null");
    const uint32_t rec = wire_record_bytes(c);
    const size_t out_cap = out_cap_bytes / rec;
    size_t total = 0;
    int rc = batch_to_device(c, frames, num_frames, frame_stride, row_stride, time_spanned, out_cap, &total);
    if (n_events) *n_events = total;
    if (n_bytes) *n_bytes = total * rec;
    if (rc != ADDER_OK) return rc;
    void *vp = c->d_wire;
    if ((rc = ensure(c, &vp, &c->d_wire_cap, std::max<size_t>(total * rec, 16))) != ADDER_OK) return rc;
    c->d_wire = (uint8_t *)vp;
    HIPCHK(c, adder_launch_wire(reinterpret_cast<const AdderEventPod *>(c->d_events), total, rec, c->d_wire, c->status,
                                c->stream));
    if (total) HIPCHK(c, hipMemcpyAsync(out_bytes, c->d_wire, total * rec, hipMemcpyDeviceToHost, c->stream));
    if (frame_offsets)
        HIPCHK(c, hipMemcpyAsync(frame_offsets, c->d_offsets, ((size_t)num_frames + 1) * sizeof(uint64_t),
                                 hipMemcpyDeviceToHost, c->stream));
    uint32_t st = 0;
    HIPCHK(c, hipMemcpyAsync(&st, c->status, sizeof st, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return status_to_code(c, st);
}

static bool device_visible_host(const void *p, void **dev) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    if (a.type != hipMemoryTypeHost || !a.devicePointer) return false;
    *dev = a.devicePointer;
    return true;
}

extern "C" int adder_hip_integrate(AdderHipCtx *c, const uint8_t *frame, size_t row_stride, float time_spanned,
                                   AdderEvent *out, size_t out_cap, size_t *n_out, uint32_t *chunk_offsets) {
    if (!c) return ADDER_E_BAD_PARAMS;
    if (n_out) *n_out = 0;
    // a buffer that holds the frame's worst case needs no rollback: submit + collect, the events sent straight
    // into `out` when the device can see it (adder_hip_alloc_pinned / hipHostRegister), else through a slot
    if (out && c->f_submitted == c->f_collected && !c->pending && c->submitted == c->collected && !c->poisoned &&
        !band_features(c) && time_spanned >= 0.0f && out_cap >= worst_case_events_per_frame(c, time_spanned)) {
        void *dev = nullptr;
        const bool direct = device_visible_host(out, &dev);
        int rc = frame_submit_impl(c, frame, row_stride, time_spanned, direct ? (AdderEvent *)dev : nullptr, out_cap);
        if (rc != ADDER_OK) return rc;
        const AdderEvent *ev = nullptr;
        const uint32_t *ch = nullptr;
        size_t n = 0;
        rc = frame_collect_impl(c, &ev, &n, &ch);
        if (n_out) *n_out = n;
        if (rc != ADDER_OK) return rc;
        if (!direct && n) memcpy(out, ev, n * sizeof(AdderEvent));
        if (chunk_offsets) memcpy(chunk_offsets, ch, ((size_t)c->num_chunks + 1) * sizeof(uint32_t));
        return ADDER_OK;
    }
    size_t n = 0;
    int rc = adder_hip_integrate_batch(c, frame, 1, 0, row_stride, time_spanned, out, out_cap, &n, nullptr);
    if (n_out) *n_out = n;
    if (rc != ADDER_OK) return rc;
    if (chunk_offsets) {
        // events are in raster order, so chunk boundaries are boundaries in y: a binary search per chunk
        size_t lo = 0;
        for (uint32_t ch = 0; ch < c->num_chunks; ++ch) {
            const uint32_t y0 = c->p.row_begin + ch * c->p.chunk_rows;
            size_t hi = n;
            while (lo < hi) {
                const size_t mid = lo + (hi - lo) / 2;
                if (out[mid].y < y0)
                    lo = mid + 1;
                else
                    hi = mid;
            }
            chunk_offsets[ch] = (uint32_t)lo;
        }
        chunk_offsets[c->num_chunks] = (uint32_t)n;
    }
    return ADDER_OK;
}

extern "C" void *adder_hip_alloc_pinned(size_t bytes) {
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}

extern "C" void adder_hip_free_pinned(void *p) {
    if (p) (void)hipHostFree(p);
}

extern "C" int adder_hip_selftest_division(uint64_t *mismatches) {
    if (!mismatches) return ADDER_E_BAD_PARAMS;
    unsigned long long *d = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&d), sizeof(*d));
    if (e == hipSuccess) e = hipMemset(d, 0, sizeof(*d));
    if (e == hipSuccess) e = adder_launch_divtest(d, nullptr);
    unsigned long long h = 0;
    if (e == hipSuccess) e = hipMemcpy(&h, d, sizeof(h), hipMemcpyDeviceToHost);
    if (d) (void)hipFree(d);
    if (e != hipSuccess) {
        g_create_error = std::string("division self-test failed to run: ") + hipGetErrorString(e);
        return ADDER_E_HIP;
    }
    *mismatches = h;
    return ADDER_OK;
}

extern "C" int adder_hip_synth_clip_device(uint8_t *d_dst, int content, uint64_t seed, uint32_t width,
                                           uint32_t height, uint32_t channels, uint32_t row_begin, uint32_t rows,
                                           uint32_t frame_begin, uint32_t num_frames, void *stream) {
    if (!d_dst || content < 0 || content > 2 || !width || !height || !channels) return ADDER_E_BAD_PARAMS;
    hipError_t e = adder_launch_synth(d_dst, content, seed, width, height, channels, row_begin, rows, frame_begin,
                                      num_frames, (hipStream_t)stream);
    if (e != hipSuccess) {
        g_create_error = std::string("synth launch failed: ") + hipGetErrorString(e);
        return ADDER_E_HIP;
    }
    return ADDER_OK;
}

extern "C" int adder_hip_check_status(AdderHipCtx *c, void *stream) {
    if (!c) return ADDER_E_BAD_PARAMS;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    uint32_t st = 0;
    HIPCHK(c, hipMemcpyAsync(&st, c->status, sizeof st, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return status_to_code(c, st);
}
