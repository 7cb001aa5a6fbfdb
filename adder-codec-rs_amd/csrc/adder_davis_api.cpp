// adder_davis_api.cpp -- C-ABI of the DAVIS -> ADDER transcoder (include/adder_davis.h): the packet bookkeeping of
// Davis::consume, the per-pixel camera state and push scratch in HBM, the launches of adder_davis.hip, the inner
// context, and the CPU forms of the chain (the same functions the kernels run).  No CPU fallback for the push.
#include <hip/hip_runtime.h>

#include <climits>
#include <new>
#include <utility>
#include <vector>

#include "../../include/adder_davis.h"
#include "adder_davis_kernels.h"
#include "adder_davis_logic.hpp"
#include "adder_source_util.hpp"

using namespace adder;

static thread_local std::string g_davis_create_error;

namespace {

enum Phase { kOpen = 0, kFinished = 1 };

}  // namespace

struct AdderDavis {
    AdderDavisParams p{};
    AdderHipCtx *ctx = nullptr;
    DavisArgs a{};
    hipStream_t stream = nullptr;  // the host-pointer forms' stream
    int phase = kOpen;
    uint64_t eps = 0;              // events one step can make at most
    // camera state: planes[cur] is committed, the other one is a push's working copy
    DavisPlanes planes[2]{};
    int cur = 0;
    // Davis's packet fields
    bool have_last_after = false;
    int64_t end_of_last = 0;
    uint64_t last_frame_events = 0;
    // the previous packet's `after` events (device), and a second buffer the next ones are copied into
    AdderDavisEvent *held = nullptr, *held2 = nullptr;
    uint64_t held_n = 0, held_cap = 0, held2_cap = 0;
    DavisScratch s{};  // push scratch
    size_t order_bytes = 0, sorted_bytes = 0;  // of s.order and s.sorted, which follow s.chain.cap
    StepBuffer steps;
    uint8_t *img = nullptr;        // Framed: image_8u
    uint64_t *frame_offs = nullptr;  // Framed: the dense batch's two offsets
    DavisScalars *h_sc = nullptr;  // pinned
    // host-pointer forms
    void *d_frame = nullptr, *d_before = nullptr, *d_after = nullptr, *d_out = nullptr;
    size_t d_frame_cap = 0, d_before_cap = 0, d_after_cap = 0, d_out_cap = 0;
    std::string err;
};

static int dfail(AdderDavis *v, int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    api_fail(v ? v->err : g_davis_create_error, code, fmt, ap);
    va_end(ap);
    return code;
}

#define DHIPCHK(v, expr) ADDER_HIPCHK(dfail, v, expr, #expr)

// ------------------------------------------------------------------------------------------ lifecycle
static void davis_free(AdderDavis *v) {
    if (!v) return;
    (void)hipSetDevice(v->p.device_id);
    if (v->stream) (void)hipStreamSynchronize(v->stream);
    (void)hipDeviceSynchronize();
    chain_free(v->s.chain);
    api_free_all({v->planes[0].ts, v->planes[0].ln, v->planes[1].ts, v->planes[1].ln, v->s.order, v->s.sorted, v->s.gcnt,
                  v->s.goffs, v->s.gstage, v->s.sc, v->held, v->held2, v->steps.p, v->img, v->frame_offs, v->d_frame,
                  v->d_before, v->d_after, v->d_out});
    if (v->h_sc) (void)hipHostFree(v->h_sc);
    if (v->ctx) adder_hip_destroy(v->ctx);
    if (v->stream) (void)hipStreamDestroy(v->stream);
    delete v;
}

// Davis::new (davis.rs:109-177) + time_parameters + .crf(c) as the mirror's Video makes its context; the camera state
// back to last ts = 0, last ln = 0.0
static int open_ctx(AdderDavis *v) {
    const AdderDavisParams &p = v->p;
    AdderHipParams hp;
    adder_hip_default_params(&hp, p.width, p.height, 1);
    hp.pixel_mode = p.mode == ADDER_DAVIS_FRAMED ? ADDER_MODE_FRAME_PERFECT : ADDER_MODE_CONTINUOUS;
    hp.ref_time = p.ref_time;
    hp.delta_t_max = p.delta_t_max;
    hp.chunk_rows = p.height / 4u;
    hp.device_id = p.device_id;
    // ADDER_DAVIS_NO_CRF (-1) leaves the context's default limits and baseline alone
    const int rc = source_open_ctx(&v->ctx, hp, p.crf, p.crf, v->a.units, &v->eps, v->err);
    if (rc != ADDER_OK) return rc;
    const size_t u = v->a.units;
    DHIPCHK(v, hipMemsetAsync(v->planes[0].ts, 0, u * 8u, v->stream));
    DHIPCHK(v, hipMemsetAsync(v->planes[0].ln, 0, u * 8u, v->stream));  // 0.0
    DHIPCHK(v, hipStreamSynchronize(v->stream));
    v->cur = 0;
    v->phase = kOpen;
    v->have_last_after = false;
    v->end_of_last = 0;
    v->held_n = 0;
    v->last_frame_events = 0;
    return ADDER_OK;
}

extern "C" int adder_davis_create(const AdderDavisParams *p, AdderDavis **out) {
    if (!p || !out) return dfail(nullptr, ADDER_E_BAD_PARAMS, "null argument");
    *out = nullptr;
    if (p->abi_version != ADDER_DAVIS_ABI_VERSION)
        return dfail(nullptr, ADDER_E_BAD_PARAMS, "abi_version %u, this library is %u", p->abi_version,
                     ADDER_DAVIS_ABI_VERSION);
    if (p->width == 0 || p->height == 0) return dfail(nullptr, ADDER_E_BAD_PARAMS, "plane %ux%u", p->width, p->height);
    if (p->height % 4u != 0u)
        return dfail(nullptr, ADDER_E_BAD_PARAMS, "height %u is not a multiple of 4 (the reference indexes four event "
                     "chunks by y / (height / 4))", p->height);
    if (p->mode < ADDER_DAVIS_FRAMED || p->mode > ADDER_DAVIS_RAW_DVS)
        return dfail(nullptr, ADDER_E_BAD_PARAMS, "mode %d", p->mode);
    if (p->ref_time == 0 || p->delta_t_max < p->ref_time || p->tps == 0)
        return dfail(nullptr, ADDER_E_BAD_PARAMS, "tps %u, ref_time %u, delta_t_max %u", p->tps, p->ref_time, p->delta_t_max);
    if (p->crf != ADDER_DAVIS_NO_CRF && (p->crf < 0 || p->crf > 9))
        return dfail(nullptr, ADDER_E_BAD_PARAMS, "crf %d (0..9, or ADDER_DAVIS_NO_CRF)", p->crf);
    if (const int rc = api_check_device(p->device_id, g_davis_create_error)) return rc;
    AdderDavis *v = new (std::nothrow) AdderDavis();
    if (!v) return dfail(nullptr, ADDER_E_BAD_PARAMS, "out of host memory");
    v->p = *p;
    DavisArgs &a = v->a;
    a.width = p->width;
    a.height = p->height;
    a.units = (uint32_t)p->width * p->height;
    a.chunk_h = p->height / 4u;
    a.key_bits = key_bits_for(a.units);
    a.mode = p->mode;
    a.tps = p->tps;
    a.ref_time = p->ref_time;
    const size_t u = a.units;
    int rc = ADDER_OK;
    auto mk = [&](void **b, size_t bytes) {
        if (rc == ADDER_OK && hipMalloc(b, bytes) != hipSuccess) rc = ADDER_E_HIP;
    };
    if (hipSetDevice(p->device_id) != hipSuccess) rc = ADDER_E_HIP;
    for (int k = 0; k < 2; ++k) {
        mk((void **)&v->planes[k].ts, u * 8u);
        mk((void **)&v->planes[k].ln, u * 8u);
    }
    mk((void **)&v->s.gcnt, u * 4u);
    mk((void **)&v->s.goffs, u * 4u);
    mk((void **)&v->s.gstage, u * sizeof(AdderSparseStep));
    mk((void **)&v->s.sc, sizeof(DavisScalars));
    mk((void **)&v->img, u);
    mk((void **)&v->frame_offs, 2u * sizeof(uint64_t));
    if (rc == ADDER_OK && hipHostMalloc((void **)&v->h_sc, sizeof(DavisScalars), hipHostMallocDefault) != hipSuccess)
        rc = ADDER_E_HIP;
    if (rc == ADDER_OK && hipStreamCreateWithFlags(&v->stream, hipStreamNonBlocking) != hipSuccess) rc = ADDER_E_HIP;
    if (rc != ADDER_OK) {
        davis_free(v);
        return dfail(nullptr, rc, "device allocation for %zu pixels failed", u);
    }
    if ((rc = open_ctx(v)) != ADDER_OK) {
        g_davis_create_error = v->err;
        davis_free(v);
        return rc;
    }
    *out = v;
    return ADDER_OK;
}

extern "C" void adder_davis_destroy(AdderDavis *v) { davis_free(v); }

extern "C" int adder_davis_reset(AdderDavis *v) {
    if (!v) return ADDER_E_BAD_PARAMS;
    DHIPCHK(v, hipSetDevice(v->p.device_id));
    DHIPCHK(v, hipDeviceSynchronize());
    return open_ctx(v);
}

extern "C" const char *adder_davis_last_error(const AdderDavis *v) {
    return v ? v->err.c_str() : g_davis_create_error.c_str();
}

extern "C" uint64_t adder_davis_events_per_step(const AdderDavis *v) { return v ? v->eps : 0; }

static uint64_t list_events(const AdderDavis *v, uint64_t n_before) {
    return v->p.mode == ADDER_DAVIS_FRAMED ? 0u : (v->have_last_after ? v->held_n : 0u) + n_before;
}

extern "C" uint64_t adder_davis_push_capacity(const AdderDavis *v, uint64_t n_before) {
    return v ? (2u * list_events(v, n_before) + 2u * (uint64_t)v->a.units) * v->eps : 0;
}

extern "C" int adder_davis_pixel_state(AdderDavis *v, int64_t *last_ts, double *last_ln) {
    if (!v) return ADDER_E_BAD_PARAMS;
    DHIPCHK(v, hipSetDevice(v->p.device_id));
    // (every push and finish has waited for its stream before it returned)
    const DavisPlanes &c = v->planes[v->cur];
    if (last_ts) DHIPCHK(v, hipMemcpy(last_ts, c.ts, (size_t)v->a.units * 8u, hipMemcpyDeviceToHost));
    if (last_ln) DHIPCHK(v, hipMemcpy(last_ln, c.ln, (size_t)v->a.units * 8u, hipMemcpyDeviceToHost));
    return ADDER_OK;
}

extern "C" int adder_davis_running_intensities(AdderDavis *v, uint8_t *dst) {
    if (!v || !dst) return ADDER_E_BAD_PARAMS;
    const int rc = adder_hip_running_intensities(v->ctx, dst);
    return rc == ADDER_OK ? rc : dfail(v, rc, "%s", adder_hip_last_error(v->ctx));
}

// ------------------------------------------------------------------------------------------ push, finish
static int ensure_scratch(AdderDavis *v, uint64_t n) {
    DavisScratch &s = v->s;
    DHIPCHK(v, chain_reserve(s.chain, n, v->a.units));  // before any list came: the gap scan's temp alone
    DHIPCHK(v, api_grow((void **)&s.order, &v->order_bytes, s.chain.cap * 4u));
    DHIPCHK(v, api_grow((void **)&s.sorted, &v->sorted_bytes, s.chain.cap * sizeof(DavisWalkEvent)));
    DHIPCHK(v, steps_reserve(v->steps, 2u * s.chain.cap + 2u * (uint64_t)v->a.units));
    return ADDER_OK;
}

static int push(AdderDavis *v, const double *d_frame, const AdderDavisMeta *meta, const AdderDavisEvent *d_before,
                uint64_t n_before, const AdderDavisEvent *d_after, uint64_t n_after, AdderEvent *d_out, uint64_t out_cap,
                uint64_t *n_out, uint64_t *bad_index, hipStream_t s) {
    if (n_out) *n_out = 0;
    if (bad_index) *bad_index = ADDER_DAVIS_NO_BAD_EVENT;
    if (v->phase != kOpen) return dfail(v, ADDER_DAVIS_E_ORDER, "push after finish (reset first)");
    if (!meta) return dfail(v, ADDER_E_BAD_PARAMS, "null meta");
    const int mode = v->p.mode;
    const bool raw = mode != ADDER_DAVIS_FRAMED;
    if (raw && !meta->has_events)
        return dfail(v, ADDER_E_BAD_PARAMS, "a packet without events in a raw mode");
    if (!raw) n_before = n_after = 0;  // Framed never looks at them
    if (mode != ADDER_DAVIS_RAW_DVS && !d_frame) return dfail(v, ADDER_E_BAD_PARAMS, "null frame");
    if ((n_before && !d_before) || (n_after && !d_after)) return dfail(v, ADDER_E_BAD_PARAMS, "null events");
    if (((uintptr_t)d_before | (uintptr_t)d_after | (uintptr_t)d_frame) & 7u)
        return dfail(v, ADDER_E_BAD_PARAMS, "the frame and the events must be 8-byte aligned");
    if (out_cap > 0 && !d_out) return dfail(v, ADDER_E_BAD_PARAMS, "null output with capacity");
    const uint64_t n = list_events(v, n_before);
    if (n + n_after > (uint64_t)INT32_MAX)
        return dfail(v, ADDER_E_BAD_PARAMS, "%llu events in one push (at most 2^31 - 1)", (unsigned long long)(n + n_after));
    const uint64_t need = adder_davis_push_capacity(v, n_before);
    if (out_cap < need) {
        if (n_out) *n_out = need;
        return dfail(v, ADDER_E_OUT_CAPACITY, "the packet may make %llu events; the buffer holds %llu",
                     (unsigned long long)need, (unsigned long long)out_cap);
    }
    DHIPCHK(v, hipSetDevice(v->p.device_id));
    int rc = ensure_scratch(v, n);
    if (rc != ADDER_OK) return rc;
    // step 1 (davis.rs:668-699)
    DavisPacket pk{};
    pk.c = meta->c;  // (RawDvs sets 0.15 after the frame, :829; the next packet's c replaces it before any use)
    pk.start = meta->has_events ? meta->img_start_ts : 0;
    pk.end = meta->has_events ? meta->img_end_ts : (int64_t)v->p.ref_time;
    if (mode == ADDER_DAVIS_RAW_DVS) pk.end = davis_delta(pk.start, -1);  // start + 1
    pk.end_of_last = v->end_of_last;
    pk.held_check2 = mode != ADDER_DAVIS_RAW_DVS ? 1 : 0;
    pk.held = v->held;
    pk.n_held = raw && v->have_last_after ? v->held_n : 0u;
    pk.before = d_before;
    pk.n_before = n_before;
    pk.after = d_after;
    pk.n_after = n_after;
    pk.frame = d_frame;
    const DavisPlanes &cur = v->planes[v->cur], &work = v->planes[v->cur ^ 1];
    const size_t u = v->a.units;
    DHIPCHK(v, hipMemcpyAsync(work.ts, cur.ts, u * 8u, hipMemcpyDeviceToDevice, s));
    DHIPCHK(v, hipMemcpyAsync(work.ln, cur.ln, u * 8u, hipMemcpyDeviceToDevice, s));
    DHIPCHK(v, davis_generate(v->a, pk, work, v->s, v->steps.p, v->img, s));
    DHIPCHK(v, hipMemcpyAsync(v->h_sc, v->s.sc, sizeof(DavisScalars), hipMemcpyDeviceToHost, s));
    // the new `after` events go to the spare buffer meanwhile; it becomes the held one only if the push is accepted
    if (raw && n_after) {
        if (n_after > v->held2_cap) {
            DHIPCHK(v, hipStreamSynchronize(s));
            if (v->held2) DHIPCHK(v, hipFree(v->held2));
            v->held2 = nullptr;
            v->held2_cap = 0;
            DHIPCHK(v, hipMalloc((void **)&v->held2, (n_after + n_after / 8u) * sizeof(AdderDavisEvent)));
            v->held2_cap = n_after + n_after / 8u;
        }
        DHIPCHK(v, hipMemcpyAsync(v->held2, d_after, n_after * sizeof(AdderDavisEvent), hipMemcpyDeviceToDevice, s));
    }
    DHIPCHK(v, hipStreamSynchronize(s));
    const DavisScalars sc = *v->h_sc;
    if (sc.bad != ~0ull) {
        if (bad_index) *bad_index = sc.bad;
        return dfail(v, ADDER_DAVIS_E_BAD_EVENT, "event %llu of the packet (`before` first) is outside the %ux%u plane",
                     (unsigned long long)sc.bad, v->a.width, v->a.height);
    }
    if (sc.bad_frame != ~0ull)
        return dfail(v, ADDER_E_BAD_PARAMS, "frame value %llu is NaN or <= -1", (unsigned long long)sc.bad_frame);
    // from here on the inner context advances: a failure leaves only reset
    uint64_t total = 0;
    size_t got = 0;
    v->last_frame_events = 0;
    if (raw) {
        // the lists' and the gaps' steps, then the frame's: two calls, so that the frame's events can be told apart
        const uint64_t head = sc.ev_steps + sc.gap_steps;
        if (head) {
            rc = adder_hip_integrate_sparse_device(v->ctx, v->steps.p, head, d_out, out_cap, &got, s);
            total = got;
        }
        if (rc == ADDER_OK) {
            got = 0;
            rc = adder_hip_integrate_sparse_device(v->ctx, v->steps.p + head, u, d_out + total, out_cap - total, &got, s);
            total += got;
            v->last_frame_events = got;
        }
        if (rc != ADDER_OK) {
            v->phase = kFinished;
            return dfail(v, rc, "integrate_sparse: %s", adder_hip_last_error(v->ctx));
        }
    } else {
        rc = adder_hip_integrate_device(v->ctx, v->img, 1, (float)v->p.ref_time, d_out, out_cap, v->frame_offs, s);
        if (rc == ADDER_OK) rc = adder_hip_finish(v->ctx, &got);
        if (rc != ADDER_OK) {
            v->phase = kFinished;
            return dfail(v, rc, "integrate: %s", adder_hip_last_error(v->ctx));
        }
        total = got;
        v->last_frame_events = got;
    }
    v->cur ^= 1;  // the commit
    if (raw) {
        std::swap(v->held, v->held2);
        std::swap(v->held_cap, v->held2_cap);
        v->held_n = n_after;
        v->have_last_after = true;
        v->end_of_last = pk.end;
    }
    if (n_out) *n_out = total;
    return ADDER_OK;
}

extern "C" int adder_davis_push_device(AdderDavis *v, const double *d_frame, const AdderDavisMeta *meta,
                                       const AdderDavisEvent *d_before, uint64_t n_before, const AdderDavisEvent *d_after,
                                       uint64_t n_after, AdderEvent *d_out, uint64_t out_cap, uint64_t *n_out,
                                       uint64_t *bad_index, void *stream) {
    if (!v) return ADDER_E_BAD_PARAMS;
    return push(v, d_frame, meta, d_before, n_before, d_after, n_after, d_out, out_cap, n_out, bad_index,
                (hipStream_t)stream);
}

extern "C" int adder_davis_push_host(AdderDavis *v, const double *frame, const AdderDavisMeta *meta,
                                     const AdderDavisEvent *before, uint64_t n_before, const AdderDavisEvent *after,
                                     uint64_t n_after, AdderEvent *out, uint64_t out_cap, uint64_t *n_out,
                                     uint64_t *bad_index) {
    if (!v) return ADDER_E_BAD_PARAMS;
    if (n_out) *n_out = 0;
    if (bad_index) *bad_index = ADDER_DAVIS_NO_BAD_EVENT;
    if (v->phase != kOpen) return dfail(v, ADDER_DAVIS_E_ORDER, "push after finish (reset first)");
    if (v->p.mode == ADDER_DAVIS_FRAMED) n_before = n_after = 0;
    if ((n_before && !before) || (n_after && !after)) return dfail(v, ADDER_E_BAD_PARAMS, "null events");
    if (out_cap > 0 && !out) return dfail(v, ADDER_E_BAD_PARAMS, "null output");
    if (n_before > (uint64_t)INT32_MAX || n_after > (uint64_t)INT32_MAX)
        return dfail(v, ADDER_E_BAD_PARAMS, "too many events in one push");
    DHIPCHK(v, hipSetDevice(v->p.device_id));
    const uint64_t most = adder_davis_push_capacity(v, n_before);
    const uint64_t dcap = out_cap < most ? out_cap : most;
    const size_t fbytes = frame ? (size_t)v->a.units * 8u : 0u;
    DHIPCHK(v, api_stage_input(&v->d_frame, &v->d_frame_cap, frame, fbytes, v->stream));
    DHIPCHK(v, api_stage_input(&v->d_before, &v->d_before_cap, before, n_before * sizeof(AdderDavisEvent), v->stream));
    DHIPCHK(v, api_stage_input(&v->d_after, &v->d_after_cap, after, n_after * sizeof(AdderDavisEvent), v->stream));
    DHIPCHK(v, api_grow(&v->d_out, &v->d_out_cap, dcap * sizeof(AdderEvent) + 16u));
    uint64_t got = 0;
    const int rc = push(v, frame ? (const double *)v->d_frame : nullptr, meta,
                        n_before ? (const AdderDavisEvent *)v->d_before : nullptr, n_before,
                        n_after ? (const AdderDavisEvent *)v->d_after : nullptr, n_after, (AdderEvent *)v->d_out, dcap, &got,
                        bad_index, v->stream);
    if (n_out) *n_out = got;
    if (rc == ADDER_OK && got) DHIPCHK(v, hipMemcpy(out, v->d_out, got * sizeof(AdderEvent), hipMemcpyDeviceToHost));
    return rc;
}

extern "C" int adder_davis_finish_device(AdderDavis *v, AdderEvent *d_out, uint64_t out_cap, uint64_t *n_out, void *stream) {
    if (!v) return ADDER_E_BAD_PARAMS;
    if (n_out) *n_out = 0;
    if (v->phase != kOpen) return dfail(v, ADDER_DAVIS_E_ORDER, "finish twice (reset first)");
    if (v->p.mode == ADDER_DAVIS_FRAMED) {  // davis.rs:641-669 pops nothing in Framed
        v->phase = kFinished;
        return ADDER_OK;
    }
    const uint64_t need = (uint64_t)v->a.units * v->eps;
    if (!d_out || out_cap < need) {
        if (n_out) *n_out = need;
        return dfail(v, ADDER_E_OUT_CAPACITY, "the flush may make %llu events", (unsigned long long)need);
    }
    DHIPCHK(v, hipSetDevice(v->p.device_id));
    const hipStream_t s = (hipStream_t)stream;
    DHIPCHK(v, steps_reserve(v->steps, v->a.units));
    DHIPCHK(v, davis_flush_steps(v->a, v->steps.p, s));
    size_t got = 0;
    const int rc = adder_hip_integrate_sparse_device(v->ctx, v->steps.p, v->a.units, d_out, out_cap, &got, s);
    v->phase = kFinished;
    if (rc != ADDER_OK) return dfail(v, rc, "integrate_sparse: %s", adder_hip_last_error(v->ctx));
    v->held_n = 0;
    if (n_out) *n_out = got;
    return ADDER_OK;
}

extern "C" int adder_davis_finish_host(AdderDavis *v, AdderEvent *out, uint64_t out_cap, uint64_t *n_out) {
    if (!v) return ADDER_E_BAD_PARAMS;
    if (n_out) *n_out = 0;
    if (v->phase != kOpen) return dfail(v, ADDER_DAVIS_E_ORDER, "finish twice (reset first)");
    if (v->p.mode == ADDER_DAVIS_FRAMED) return adder_davis_finish_device(v, nullptr, 0, n_out, nullptr);
    const uint64_t need = (uint64_t)v->a.units * v->eps;
    if (!out || out_cap < need) {
        if (n_out) *n_out = need;
        return dfail(v, ADDER_E_OUT_CAPACITY, "the flush may make %llu events", (unsigned long long)need);
    }
    DHIPCHK(v, hipSetDevice(v->p.device_id));
    DHIPCHK(v, api_grow(&v->d_out, &v->d_out_cap, need * sizeof(AdderEvent)));
    uint64_t got = 0;
    const int rc = adder_davis_finish_device(v, (AdderEvent *)v->d_out, need, &got, v->stream);
    if (rc != ADDER_OK) return rc;
    if (got) DHIPCHK(v, hipMemcpy(out, v->d_out, got * sizeof(AdderEvent), hipMemcpyDeviceToHost));
    if (n_out) *n_out = got;
    return ADDER_OK;
}

extern "C" uint64_t adder_davis_last_frame_events(const AdderDavis *v) { return v ? v->last_frame_events : 0; }

// ------------------------------------------------------------------------------------------ the chain on the CPU
extern "C" int adder_davis_steps_host(uint16_t width, uint16_t height, int64_t *last_ts, double *last_ln,
                                      const AdderDavisEvent *events, uint64_t n, int64_t check1, int32_t check2_mode,
                                      int64_t check2, double c, uint32_t tps, uint32_t ref_time, AdderSparseStep *steps,
                                      uint64_t steps_cap, uint64_t *n_steps, uint64_t *bad_index) {
    if (n_steps) *n_steps = 0;
    if (bad_index) *bad_index = ADDER_DAVIS_NO_BAD_EVENT;
    if (!last_ts || !last_ln || (n && !events) || width == 0 || height == 0 || height % 4u != 0u || ref_time == 0 ||
        check2_mode < 0 || check2_mode > 2)
        return ADDER_E_BAD_PARAMS;
    for (uint64_t i = 0; i < n; ++i)
        if (events[i].x >= width || events[i].y >= height) {
            if (bad_index) *bad_index = i;
            return ADDER_DAVIS_E_BAD_EVENT;
        }
    if (steps_cap < 2u * n || (n && !steps)) {
        if (n_steps) *n_steps = 2u * n;
        return ADDER_E_OUT_CAPACITY;
    }
    const DavisConsts k = davis_consts(c, tps, ref_time);
    const uint32_t chunk_h = height / 4u;
    uint64_t made = 0;
    // the four row chunks one after the other, arrival order inside a chunk (davis.rs:254-258)
    for (uint32_t chunk = 0; chunk < 4u; ++chunk)
        for (uint64_t i = 0; i < n; ++i) {
            const AdderDavisEvent &e = events[i];
            if (e.y / chunk_h != chunk || !davis_event_passes(e.t, check1, check2_mode, check2)) continue;
            const size_t p = (size_t)e.y * width + e.x;
            DavisPixel px = davis_pixel(last_ts[p], last_ln[p]);
            made += davis_event_steps(px, e.x, e.y, e.t, e.on != 0, k, steps + made);
            last_ts[p] = px.ts;
            last_ln[p] = px.ln;
        }
    if (n_steps) *n_steps = made;
    return ADDER_OK;
}

extern "C" int adder_davis_gaps_host(uint16_t width, uint16_t height, const int64_t *last_ts, double *last_ln, int64_t start,
                                     uint32_t tps, uint32_t ref_time, AdderSparseStep *steps, uint64_t steps_cap,
                                     uint64_t *n_steps) {
    if (n_steps) *n_steps = 0;
    if (!last_ts || !last_ln || width == 0 || height == 0 || ref_time == 0) return ADDER_E_BAD_PARAMS;
    const size_t units = (size_t)width * height;
    if (steps_cap < units || !steps) {
        if (n_steps) *n_steps = units;
        return ADDER_E_OUT_CAPACITY;
    }
    const DavisConsts k = davis_consts(0.0, tps, ref_time);
    uint64_t made = 0;
    for (size_t p = 0; p < units; ++p)
        made += davis_gap_step(last_ts[p], last_ln[p], (uint32_t)(p % width), (uint32_t)(p / width), start, k, steps + made);
    if (n_steps) *n_steps = made;
    return ADDER_OK;
}

extern "C" int adder_davis_frame_host(uint16_t width, uint16_t height, int32_t mode, const double *frame, int64_t start,
                                      int64_t end, int64_t *last_ts, double *last_ln, uint8_t *image_8u,
                                      AdderSparseStep *steps) {
    if (!last_ln || width == 0 || height == 0 || mode < ADDER_DAVIS_FRAMED || mode > ADDER_DAVIS_RAW_DVS)
        return ADDER_E_BAD_PARAMS;
    const bool raw = mode != ADDER_DAVIS_FRAMED;
    if ((mode != ADDER_DAVIS_RAW_DVS && !frame) || (raw && (!steps || !last_ts))) return ADDER_E_BAD_PARAMS;
    const size_t units = (size_t)width * height;
    if (mode != ADDER_DAVIS_RAW_DVS)
        for (size_t p = 0; p < units; ++p)
            if (!davis_frame_value_ok(frame[p])) return ADDER_E_BAD_PARAMS;
    const float span = davis_frame_span(mode, start, end, 0u);
    for (size_t p = 0; p < units; ++p) {
        const uint8_t b = davis_frame_pixel(mode, mode != ADDER_DAVIS_RAW_DVS ? frame[p] : 0.0, last_ln[p]);
        if (image_8u) image_8u[p] = b;
        if (raw) {
            last_ts[p] = end;
            steps[p] = davis_step((uint32_t)(p % width), (uint32_t)(p / width), b, 0u, (float)b, span);
        }
    }
    return ADDER_OK;
}
