// adder_viz_player_api.cpp -- C-ABI of the adder-viz player (include/adder_viz_player.h): the carried state and call
// scratch in HBM, the launches of adder_viz_player.hip, and the scalars of the schedule (frames_written, M, the global
// event count), which live on the host: every call waits for its stream anyway.  No CPU fallback.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <new>
#include <numeric>
#include <vector>

#include "../../include/adder_viz_player.h"
#include "adder_api_util.hpp"
#include "adder_feature_intervals.hpp"
#include "adder_viz_player_features.hpp"
#include "adder_viz_player_kernels.h"
#include "adder_viz_player_logic.hpp"
#include "adder_wire.hpp"

using namespace adder;

static thread_local std::string g_viz_create_error;

struct AdderVizPlayer {
    AdderVizPlayerParams p{};
    VizArgs a{};
    uint32_t tpf = 0;
    int32_t frames_written = 0;
    int32_t m = -1;           // the largest last_filled any event left
    uint64_t n_events = 0;    // events ingested since creation (the global index of the next one)
    int has_limit = 0;
    uint32_t limit = 0;
    bool finished = false;
    bool limit_set = false;  // since the last call
    hipStream_t stream = nullptr;  // the host-pointer forms' stream
    uint64_t cap = 0;              // call scratch, for `cap` events
    VizScratch s{};
    VizScalars *h_sc = nullptr;  // pinned
    int32_t *h_pops = nullptr;   // pinned, ring + 1
    void *d_in = nullptr;        // host-pointer forms: the input and the frames on the device
    size_t d_in_cap = 0;
    void *d_out = nullptr;
    size_t d_out_cap = 0;
    std::string err;
    // feature detection (adder_viz_player_detect_features); the device side is allocated when it is first switched on
    bool detect = false;
    uint8_t *plane = nullptr;      // running_intensities
    bool carry_valid = false;      // the carried last event {valid, t}: host scalars, like the schedule's
    uint32_t carry_t = 0;
    uint32_t *h_tail = nullptr;    // pinned: t_after of the call's last event
    void *det_block = nullptr;     // the per-call arrays of VizDetect, carved from one allocation that only grows
    size_t det_block_cap = 0;
    FeatureIntervals intervals;    // FrameSequence::features: runs from creation, one pop per popped frame
    std::vector<AdderFramerFeature> feat_host;  // the last ingest call's features
    std::vector<int32_t> feat_w_host;
    std::vector<uint64_t> fi_end, fi_off;       // the intervals popped by the last ingest / finish call
    std::vector<uint16_t> fi_xy;
    std::vector<unsigned long long> stamps;     // its cross stamps
    void *d_stamps = nullptr;
    size_t d_stamps_cap = 0;
};

static int vfail(AdderVizPlayer *v, int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    api_fail(v ? v->err : g_viz_create_error, code, fmt, ap);
    va_end(ap);
    return code;
}

#define VHIPCHK(v, expr) ADDER_HIPCHK(vfail, v, expr, #expr)

static void free_scratch(AdderVizPlayer *v) {
    VizScratch &s = v->s;
    api_free_all({s.ukeys0, s.ukeys1, s.uidx0, s.uidx1, s.rkeys0, s.rkeys1, s.ridx0, s.ridx1, s.s_l, s.s_val, s.s_px, s.l_in,
                  s.pm, s.comb_in, s.comb, s.temp});
    VizScratch keep{};
    keep.cnt_call = s.cnt_call;
    keep.nat_call = s.nat_call;
    keep.done_new = s.done_new;
    keep.pops = s.pops;
    keep.flushed = s.flushed;
    keep.sc = s.sc;
    s = keep;
    v->cap = 0;
}

static void viz_free(AdderVizPlayer *v) {
    if (!v) return;
    (void)hipSetDevice(v->p.device_id);
    if (v->stream) (void)hipStreamSynchronize(v->stream);
    (void)hipDeviceSynchronize();
    free_scratch(v);
    api_free_all({v->a.px, v->a.ring_val, v->a.ring_some, v->a.running, v->a.cnt, v->a.done, v->a.run_lo, v->s.cnt_call,
                  v->s.nat_call, v->s.done_new, v->s.pops, v->s.flushed, v->s.sc, v->d_in, v->d_out, v->plane, v->det_block,
                  v->d_stamps});
    if (v->h_sc) (void)hipHostFree(v->h_sc);
    if (v->h_tail) (void)hipHostFree(v->h_tail);
    if (v->h_pops) (void)hipHostFree(v->h_pops);
    if (v->stream) (void)hipStreamDestroy(v->stream);
    delete v;
}

static int ensure_scratch(AdderVizPlayer *v, uint64_t n) {
    if (n <= v->cap && v->cap > 0) return ADDER_OK;
    free_scratch(v);
    uint64_t c = n + n / 8u + 1u;
    if (c > (uint64_t)INT32_MAX - 1u) c = (uint64_t)INT32_MAX - 1u;
    VizScratch &s = v->s;
    VHIPCHK(v, hipMalloc((void **)&s.ukeys0, c * 4u));
    VHIPCHK(v, hipMalloc((void **)&s.ukeys1, c * 4u));
    VHIPCHK(v, hipMalloc((void **)&s.uidx0, c * 4u));
    VHIPCHK(v, hipMalloc((void **)&s.uidx1, c * 4u));
    VHIPCHK(v, hipMalloc((void **)&s.rkeys0, c * 4u));
    VHIPCHK(v, hipMalloc((void **)&s.rkeys1, c * 4u));
    VHIPCHK(v, hipMalloc((void **)&s.ridx0, c * 4u));
    VHIPCHK(v, hipMalloc((void **)&s.ridx1, c * 4u));
    VHIPCHK(v, hipMalloc((void **)&s.s_l, c * 4u));
    VHIPCHK(v, hipMalloc((void **)&s.s_val, c));
    VHIPCHK(v, hipMalloc((void **)&s.s_px, c * sizeof(FramerPx)));
    VHIPCHK(v, hipMalloc((void **)&s.l_in, c * 4u));
    VHIPCHK(v, hipMalloc((void **)&s.pm, c * 4u));
    VHIPCHK(v, hipMalloc((void **)&s.comb_in, c * 8u));
    VHIPCHK(v, hipMalloc((void **)&s.comb, c * 8u));
    s.temp_bytes = viz_temp_bytes(c);
    VHIPCHK(v, hipMalloc(&s.temp, s.temp_bytes));
    v->cap = c;
    return ADDER_OK;
}

static int reset_state(AdderVizPlayer *v) {
    const VizArgs &a = v->a;
    const size_t u = a.units, cells = (size_t)a.height * a.ring;
    std::vector<FramerPx> init(u, FramerPx{0u, -1, 0u});  // pixel_ts 0, last_filled -1, last intensity 0
    VHIPCHK(v, hipSetDevice(v->p.device_id));
    VHIPCHK(v, hipDeviceSynchronize());
    VHIPCHK(v, hipMemcpy(a.px, init.data(), u * sizeof(FramerPx), hipMemcpyHostToDevice));
    VHIPCHK(v, hipMemset(a.ring_val, 0, u * a.ring));
    VHIPCHK(v, hipMemset(a.ring_some, 0, u * a.ring));
    VHIPCHK(v, hipMemset(a.running, 0, u));
    VHIPCHK(v, hipMemset(a.cnt, 0, cells * 4u));
    VHIPCHK(v, hipMemset(a.done, 0, a.height));
    if (v->plane) VHIPCHK(v, hipMemset(v->plane, 0, u));
    VHIPCHK(v, hipDeviceSynchronize());  // the calls run on other streams
    v->carry_valid = false;
    v->intervals.clear();
    v->feat_host.clear();
    v->feat_w_host.clear();
    v->fi_end.clear();
    v->fi_off.assign(1, 0u);
    v->fi_xy.clear();
    v->frames_written = 0;
    v->m = -1;
    v->n_events = 0;
    v->finished = false;
    v->limit_set = false;
    return ADDER_OK;
}

extern "C" int adder_viz_player_create(const AdderVizPlayerParams *pp, AdderVizPlayer **out) {
    if (!pp || !out) return vfail(nullptr, ADDER_E_BAD_PARAMS, "null argument");
    *out = nullptr;
    const AdderVizPlayerParams p = *pp;
    if (p.abi_version != ADDER_VIZ_PLAYER_ABI_VERSION)
        return vfail(nullptr, ADDER_E_BAD_PARAMS, "abi_version %u, this library is %u", p.abi_version,
                     ADDER_VIZ_PLAYER_ABI_VERSION);
    if (!p.width || !p.height || (p.channels != 1 && p.channels != 3))
        return vfail(nullptr, ADDER_E_BAD_PARAMS, "plane %ux%ux%u", p.width, p.height, p.channels);
    if (!p.ref_interval || !p.tps) return vfail(nullptr, ADDER_E_BAD_PARAMS, "tps and ref_interval must be non-zero");
    if (p.time_mode > ADDER_TIME_MIXED) return vfail(nullptr, ADDER_E_BAD_PARAMS, "bad time_mode");
    if (p.view_mode > 3 || p.source_type > 3) return vfail(nullptr, ADDER_E_BAD_PARAMS, "bad view_mode / source_type");
    if (p.has_buffer_limit && p.buffer_limit == 0)
        return vfail(nullptr, ADDER_E_BAD_PARAMS,
                     "buffer_limit 0: the reference's pop loop never ends there (a deque always holds one frame)");
    uint32_t tpf = p.ref_interval;  // FrameSequence::new (driver.rs:357-361)
    if (p.output_fps > 0.0f) {
        const float q = (float)p.tps / p.output_fps;
        tpf = q >= 4294967296.0f ? 0xffffffffu : (uint32_t)q;
    }
    if (!tpf) return vfail(nullptr, ADDER_E_BAD_PARAMS, "ticks per output frame is zero");
    const uint64_t units = (uint64_t)p.width * p.height * p.channels;
    if (units > 0x7ffffff0ull) return vfail(nullptr, ADDER_E_BAD_PARAMS, "plane too large");
    const uint64_t ring = p.ring_frames ? p.ring_frames : std::min<uint64_t>((uint64_t)p.delta_t_max / tpf + 80u, 1u << 16);
    if (ring > (1u << 16) || ring * p.height >= (1ull << 31))
        return vfail(nullptr, ADDER_E_BAD_PARAMS, "ring_frames %llu (at most 65536, and height * ring_frames < 2^31)",
                     (unsigned long long)ring);
    if (const int rc = api_check_device(p.device_id, g_viz_create_error)) return rc;
    AdderVizPlayer *v = new (std::nothrow) AdderVizPlayer();
    if (!v) return vfail(nullptr, ADDER_E_BAD_PARAMS, "out of host memory");
    v->p = p;
    v->tpf = tpf;
    v->has_limit = p.has_buffer_limit ? 1 : 0;
    v->limit = p.buffer_limit;
    VizArgs &a = v->a;
    a.width = p.width;
    a.height = p.height;
    a.channels = p.channels;
    a.units = (uint32_t)units;
    a.row_units = (uint32_t)p.width * p.channels;
    a.unit_bits = 1;
    while ((1ull << a.unit_bits) < units + 1u) ++a.unit_bits;
    a.row_bits = 1;
    while ((1ull << a.row_bits) < (uint64_t)p.height + 1u) ++a.row_bits;
    a.ring = (uint32_t)ring;
    a.k = framer_consts(tpf, p.ref_interval, (p.codec_version >= 2 && p.time_mode == ADDER_TIME_ABSOLUTE_T) ? 1u : 0u,
                        (p.codec_version >= 1 && p.source_camera <= 5u) ? 1u : 0u, p.view_mode, p.source_type,
                        p.practical_d_max, p.delta_t_max, 0u);
    const size_t u = a.units, cells = (size_t)p.height * a.ring;
    int rc = ADDER_OK;
    auto mk = [&](void **b, size_t bytes) {
        if (rc == ADDER_OK && hipMalloc(b, bytes) != hipSuccess) rc = ADDER_E_HIP;
    };
    if (hipSetDevice(p.device_id) != hipSuccess) rc = ADDER_E_HIP;
    mk((void **)&a.px, u * sizeof(FramerPx));
    mk((void **)&a.ring_val, u * a.ring);
    mk((void **)&a.ring_some, u * a.ring);
    mk((void **)&a.running, u);
    mk((void **)&a.cnt, cells * 4u);
    mk((void **)&a.done, p.height);
    mk((void **)&a.run_lo, (u + 1u) * 4u);
    mk((void **)&v->s.cnt_call, cells * 4u);
    mk((void **)&v->s.nat_call, cells * 4u);
    mk((void **)&v->s.done_new, p.height);
    mk((void **)&v->s.pops, ((size_t)a.ring + 1u) * 4u);
    mk((void **)&v->s.flushed, (size_t)a.ring + 1u);
    mk((void **)&v->s.sc, sizeof(VizScalars));
    if (rc == ADDER_OK && hipHostMalloc((void **)&v->h_sc, sizeof(VizScalars), hipHostMallocDefault) != hipSuccess)
        rc = ADDER_E_HIP;
    if (rc == ADDER_OK &&
        hipHostMalloc((void **)&v->h_pops, ((size_t)a.ring + 1u) * 4u, hipHostMallocDefault) != hipSuccess)
        rc = ADDER_E_HIP;
    if (rc == ADDER_OK && hipStreamCreateWithFlags(&v->stream, hipStreamNonBlocking) != hipSuccess) rc = ADDER_E_HIP;
    if (rc == ADDER_OK) rc = reset_state(v);
    if (rc != ADDER_OK) {
        viz_free(v);
        return vfail(nullptr, rc, "device allocation for %zu units and %u pending frames failed", u, (uint32_t)ring);
    }
    *out = v;
    return ADDER_OK;
}

extern "C" void adder_viz_player_destroy(AdderVizPlayer *v) { viz_free(v); }
extern "C" int adder_viz_player_reset(AdderVizPlayer *v) { return v ? reset_state(v) : ADDER_E_BAD_PARAMS; }
extern "C" const char *adder_viz_player_last_error(const AdderVizPlayer *v) {
    return v ? v->err.c_str() : g_viz_create_error.c_str();
}
extern "C" uint32_t adder_viz_player_tpf(const AdderVizPlayer *v) { return v ? v->tpf : 0u; }
extern "C" int64_t adder_viz_player_frames_written(const AdderVizPlayer *v) { return v ? v->frames_written : 0; }

extern "C" int adder_viz_player_set_buffer_limit(AdderVizPlayer *v, int has, uint32_t limit) {
    if (!v) return ADDER_E_BAD_PARAMS;
    if (has && limit == 0) return vfail(v, ADDER_E_BAD_PARAMS, "buffer_limit 0: the reference's pop loop never ends there");
    v->has_limit = has ? 1 : 0;
    v->limit = limit;
    v->limit_set = true;
    v->carry_valid = false;  // adaptive_state_update lies between two `consume` calls: last_event = None (adder.rs:409)
    return ADDER_OK;
}

extern "C" int adder_viz_player_detect_features(AdderVizPlayer *v, int on) {
    if (!v) return ADDER_E_BAD_PARAMS;
    if (on && !v->plane) {
        VHIPCHK(v, hipSetDevice(v->p.device_id));
        VHIPCHK(v, hipMalloc((void **)&v->plane, v->a.units));
        VHIPCHK(v, hipMemset(v->plane, 0, v->a.units));
        VHIPCHK(v, hipHostMalloc((void **)&v->h_tail, sizeof(uint32_t), hipHostMallocDefault));
        VHIPCHK(v, hipDeviceSynchronize());
    }
    v->detect = on != 0;
    v->carry_valid = false;  // a UI update lies between two `consume` calls
    return ADDER_OK;
}

static size_t det_align(size_t b) { return (b + 255u) & ~(size_t)255u; }

// the per-call arrays of a call of n events made with detection on
static int det_scratch(AdderVizPlayer *v, uint64_t n, VizDetect *d) {
    const size_t c = (size_t)n + 1u;
    size_t off = 0;
    auto carve = [&](size_t bytes) {
        const size_t at = off;
        off += det_align(bytes);
        return at;
    };
    const size_t o_val = carve(c), o_ta = carve(4u * c), o_mk = carve(c), o_fl = carve(4u * c), o_of = carve(4u * c),
                 o_ft = carve(sizeof(AdderFramerFeature) * c), o_fw = carve(4u * c);
    VHIPCHK(v, api_grow(&v->det_block, &v->det_block_cap, off));
    uint8_t *b = (uint8_t *)v->det_block;
    d->val_in = b + o_val;
    d->t_after = (uint32_t *)(b + o_ta);
    d->mark = b + o_mk;
    d->flag = (uint32_t *)(b + o_fl);
    d->offs = (uint32_t *)(b + o_of);
    d->feat = (AdderFramerFeature *)(b + o_ft);
    d->feat_w = (int32_t *)(b + o_fw);
    return ADDER_OK;
}

// The deque bookkeeping of one call, in event / pop order: a feature of event i is filed before the frames popped
// after an event >= i (under the frames_written of its period), every popped frame takes one interval.  Leaves the
// intervals in fi_* and their crosses (adder.rs:359-388: radius 2, both arms, every channel) as sorted stamps.  nf: the
// features of feat_host to file (none at finish, which keeps the last ingest call's list).
static void file_and_pop(AdderVizPlayer *v, uint32_t n_pops, size_t nf) {
    const VizArgs &a = v->a;
    v->fi_end.clear();
    v->fi_off.assign(1, 0u);
    v->fi_xy.clear();
    v->stamps.clear();
    size_t f = 0;
    auto file_until = [&](int64_t last_index) {  // global index
        for (; f < nf && (int64_t)v->feat_host[f].index <= last_index; ++f)
            v->intervals.file(v->tpf, v->feat_host[f].t, v->feat_host[f].x, v->feat_host[f].y, v->feat_w_host[f]);
    };
    for (uint32_t k = 0; k < n_pops; ++k) {
        file_until((int64_t)v->n_events + (int64_t)v->h_pops[k]);
        const FeatureInterval iv = v->intervals.pop(v->tpf);
        v->fi_end.push_back(iv.end_ts);
        for (size_t q = 0; q + 1u < iv.xy.size(); q += 2u) {
            const uint32_t x = iv.xy[q], y = iv.xy[q + 1u];
            v->fi_xy.push_back((uint16_t)x);
            v->fi_xy.push_back((uint16_t)y);
            for (int i = -2; i <= 2; ++i)
                for (uint32_t c = 0; c < a.channels; ++c) {  // never out of bounds: a feature is 3 pixels off the border
                    v->stamps.push_back(viz_stamp_key((((uint32_t)((int)y + i)) * a.width + x) * a.channels + c, k));
                    v->stamps.push_back(viz_stamp_key((y * a.width + (uint32_t)((int)x + i)) * a.channels + c, k));
                }
        }
        v->fi_off.push_back(v->fi_xy.size() / 2u);
    }
    file_until(INT64_MAX);
    std::sort(v->stamps.begin(), v->stamps.end());
}

// One call: everything up to the schedule, a wait for the pop count, then the hand-out into d_frames (device) or, when
// `h_frames` is given, into the context's own buffer and from there to the host; then the commit.
static int run(AdderVizPlayer *v, int source, const void *d_in, uint64_t n, int finish, int form, uint8_t *d_frames,
               uint8_t *h_frames, uint64_t frame_cap, uint64_t *n_frames, int64_t *pop_index, uint64_t *bad_index,
               uint64_t *n_consumed, hipStream_t stream) {
    if (!v) return ADDER_E_BAD_PARAMS;
    if (n_frames) *n_frames = 0;
    if (bad_index) *bad_index = ADDER_VIZ_PLAYER_NO_BAD_EVENT;
    if (n_consumed) *n_consumed = 0;
    if (form != ADDER_VIZ_FRAME_POPPED && form != ADDER_VIZ_FRAME_RUNNING)
        return vfail(v, ADDER_E_BAD_PARAMS, "form %d", form);
    if (v->finished) return vfail(v, ADDER_E_BAD_PARAMS, "the stream was finished: this context takes no more events");
    if (n > (uint64_t)INT32_MAX - 1u)
        return vfail(v, ADDER_E_BAD_PARAMS, "%llu records in one call (at most 2^31 - 2)", (unsigned long long)n);
    if (n > 0 && !d_in) return vfail(v, ADDER_E_BAD_PARAMS, "null input");
    if (frame_cap > 0 && !d_frames && !h_frames)
        return vfail(v, ADDER_E_BAD_PARAMS, "null frames with capacity %llu", (unsigned long long)frame_cap);
    VHIPCHK(v, hipSetDevice(v->p.device_id));
    int rc = ensure_scratch(v, n);
    if (rc != ADDER_OK) return rc;
    const VizArgs &a = v->a;
    VizDetect det{};
    if (v->detect && !finish) {
        rc = det_scratch(v, n, &det);
        if (rc != ADDER_OK) return rc;
        det.plane = v->plane;
        det.carry_valid = v->carry_valid ? 1u : 0u;
        det.carry_t = v->carry_t;
        det.index_base = v->n_events;
    }
    VHIPCHK(v, viz_prepare(a, source, d_in, n, v->frames_written, v->m, v->has_limit, v->limit,
                           v->limit_set ? 1 : 0, finish, v->s, det, stream));
    VHIPCHK(v, hipMemcpyAsync(v->h_sc, v->s.sc, sizeof(VizScalars), hipMemcpyDeviceToHost, stream));
    VHIPCHK(v, hipMemcpyAsync(v->h_pops, v->s.pops, ((size_t)a.ring + 1u) * 4u, hipMemcpyDeviceToHost, stream));
    VHIPCHK(v, hipStreamSynchronize(stream));
    const VizScalars sc = *v->h_sc;
    const bool bad = sc.bad < sc.eof;
    const uint64_t lim = bad ? sc.bad : sc.eof;
    if (sc.status & kVizStatusRange) return vfail(v, ADDER_E_BAD_PARAMS, "frame index out of range");
    if ((sc.status & kVizStatusDepth) || sc.overflow || sc.n_pops > a.ring)
        return vfail(v, ADDER_E_OUT_CAPACITY,
                     "the frame ring (%u frames) is too small for this stream: raise AdderVizPlayerParams.ring_frames",
                     a.ring);
    if (n_frames) *n_frames = sc.n_pops;
    if (sc.n_pops > frame_cap)
        return vfail(v, ADDER_E_OUT_CAPACITY, "%u frames do not fit in %llu", sc.n_pops, (unsigned long long)frame_cap);
    // From here on the call is not refused; only a HIP error can still end it, and that leaves the context unusable (the
    // header says so).  Its features come back (one more wait, with detection on only), the host files them and pops
    // one interval per frame, and the crosses go up as stamps.
    if (!finish) {
        v->feat_host.resize(det.plane ? sc.n_feat : 0u);
        v->feat_w_host.resize(v->feat_host.size());
        if (!v->feat_host.empty()) {
            VHIPCHK(v, hipMemcpyAsync(v->feat_host.data(), det.feat, v->feat_host.size() * sizeof(AdderFramerFeature),
                                      hipMemcpyDeviceToHost, stream));
            VHIPCHK(v, hipMemcpyAsync(v->feat_w_host.data(), det.feat_w, v->feat_w_host.size() * 4u, hipMemcpyDeviceToHost,
                                      stream));
            VHIPCHK(v, hipStreamSynchronize(stream));
        }
    }
    file_and_pop(v, sc.n_pops, finish ? 0u : v->feat_host.size());
    const uint32_t n_stamps = (uint32_t)v->stamps.size();
    if (n_stamps) {
        VHIPCHK(v, api_grow(&v->d_stamps, &v->d_stamps_cap, (size_t)n_stamps * 8u));
        VHIPCHK(v, hipMemcpyAsync(v->d_stamps, v->stamps.data(), (size_t)n_stamps * 8u, hipMemcpyHostToDevice, stream));
    }
    const size_t fb = a.units;
    if (h_frames) {
        VHIPCHK(v, api_grow(&v->d_out, &v->d_out_cap, (size_t)sc.n_pops * fb + 8u));
        d_frames = (uint8_t *)v->d_out;
    }
    VHIPCHK(v, viz_handout_commit(a, n, lim, v->frames_written, sc.n_pops, form, d_frames, v->s,
                                  (const unsigned long long *)v->d_stamps, n_stamps, det, stream));
    if (h_frames && sc.n_pops)
        VHIPCHK(v, hipMemcpyAsync(h_frames, d_frames, (size_t)sc.n_pops * fb, hipMemcpyDeviceToHost, stream));
    if (det.plane && lim > 0u)
        VHIPCHK(v, hipMemcpyAsync(v->h_tail, det.t_after + (lim - 1u), sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    VHIPCHK(v, hipStreamSynchronize(stream));
    if (det.plane && lim > 0u) {  // last_event, unless the call's last event ended a period
        v->carry_valid = !(sc.n_pops > 0u && (uint64_t)((int64_t)v->h_pops[sc.n_pops - 1u] + 1) == lim);
        v->carry_t = *v->h_tail;
    }
    if (pop_index)
        for (uint32_t k = 0; k < sc.n_pops; ++k) pop_index[k] = (int64_t)v->n_events + (int64_t)v->h_pops[k];
    v->frames_written = sc.w_end;
    v->m = sc.m_end;
    v->n_events += lim;
    v->limit_set = false;
    if (finish) v->finished = true;
    if (n_consumed) *n_consumed = sc.eof;
    if (bad) {
        if (bad_index) *bad_index = sc.bad;
        return vfail(v, ADDER_VIZ_PLAYER_E_BAD_EVENT, "event %llu of the batch lies outside the %ux%ux%u plane",
                     (unsigned long long)sc.bad, a.width, a.height, a.channels);
    }
    return ADDER_OK;
}

extern "C" int adder_viz_player_ingest_device(AdderVizPlayer *v, const AdderEvent *d_events, uint64_t n, int form,
                                              uint8_t *d_frames, uint64_t frame_cap, uint64_t *n_frames,
                                              int64_t *pop_index, uint64_t *bad_index, void *stream) {
    return run(v, kSrcEvents, d_events, n, 0, form, d_frames, nullptr, frame_cap, n_frames, pop_index, bad_index, nullptr,
               (hipStream_t)stream);
}

extern "C" int adder_viz_player_ingest_wire_device(AdderVizPlayer *v, const uint8_t *d_wire, uint64_t n_records, int form,
                                                   uint8_t *d_frames, uint64_t frame_cap, uint64_t *n_frames,
                                                   int64_t *pop_index, uint64_t *bad_index, uint64_t *n_consumed,
                                                   void *stream) {
    if (!v) return ADDER_E_BAD_PARAMS;
    return run(v, wire_source(v->p.channels), d_wire, n_records, 0, form, d_frames, nullptr, frame_cap, n_frames,
               pop_index, bad_index, n_consumed, (hipStream_t)stream);
}

extern "C" int adder_viz_player_finish_device(AdderVizPlayer *v, int form, uint8_t *d_frames, uint64_t frame_cap,
                                              uint64_t *n_frames, int64_t *pop_index, void *stream) {
    return run(v, kSrcEvents, nullptr, 0, 1, form, d_frames, nullptr, frame_cap, n_frames, pop_index, nullptr, nullptr,
               (hipStream_t)stream);
}

static uint8_t g_none;  // a non-null host target for a capacity of zero

static int run_host(AdderVizPlayer *v, int source, const void *in, uint64_t n, int form, uint8_t *frames,
                    uint64_t frame_cap, uint64_t *n_frames, int64_t *pop_index, uint64_t *bad_index,
                    uint64_t *n_consumed) {
    if (!v) return ADDER_E_BAD_PARAMS;
    if (n > (uint64_t)INT32_MAX - 1u) return vfail(v, ADDER_E_BAD_PARAMS, "too many records in one call");
    if (n > 0 && !in) return vfail(v, ADDER_E_BAD_PARAMS, "null input");
    if (frame_cap > 0 && !frames) return vfail(v, ADDER_E_BAD_PARAMS, "null frames");
    VHIPCHK(v, hipSetDevice(v->p.device_id));
    VHIPCHK(v, api_stage_input(&v->d_in, &v->d_in_cap, in, n * wire_record_bytes(source), v->stream));
    return run(v, source, v->d_in, n, 0, form, nullptr, frames ? frames : &g_none, frame_cap, n_frames, pop_index,
               bad_index, n_consumed, v->stream);
}

extern "C" int adder_viz_player_ingest(AdderVizPlayer *v, const AdderEvent *events, uint64_t n, int form, uint8_t *frames,
                                       uint64_t frame_cap, uint64_t *n_frames, int64_t *pop_index, uint64_t *bad_index) {
    return run_host(v, kSrcEvents, events, n, form, frames, frame_cap, n_frames, pop_index, bad_index, nullptr);
}

extern "C" int adder_viz_player_ingest_wire(AdderVizPlayer *v, const uint8_t *wire, uint64_t n_records, int form,
                                            uint8_t *frames, uint64_t frame_cap, uint64_t *n_frames, int64_t *pop_index,
                                            uint64_t *bad_index, uint64_t *n_consumed) {
    if (!v) return ADDER_E_BAD_PARAMS;
    return run_host(v, wire_source(v->p.channels), wire, n_records, form, frames, frame_cap, n_frames, pop_index,
                    bad_index, n_consumed);
}

extern "C" int adder_viz_player_finish(AdderVizPlayer *v, int form, uint8_t *frames, uint64_t frame_cap,
                                       uint64_t *n_frames, int64_t *pop_index) {
    if (!v) return ADDER_E_BAD_PARAMS;
    if (frame_cap > 0 && !frames) return vfail(v, ADDER_E_BAD_PARAMS, "null frames");
    return run(v, kSrcEvents, nullptr, 0, 1, form, nullptr, frames ? frames : &g_none, frame_cap, n_frames, pop_index,
               nullptr, nullptr, v->stream);
}

extern "C" int adder_viz_player_running_frame(AdderVizPlayer *v, uint8_t *frame) {
    if (!v) return ADDER_E_BAD_PARAMS;
    if (!frame) return vfail(v, ADDER_E_BAD_PARAMS, "null frame");
    VHIPCHK(v, hipSetDevice(v->p.device_id));
    VHIPCHK(v, hipMemcpyAsync(frame, v->a.running, v->a.units, hipMemcpyDeviceToHost, v->stream));
    VHIPCHK(v, hipStreamSynchronize(v->stream));
    return ADDER_OK;
}

extern "C" int adder_viz_player_features(AdderVizPlayer *v, AdderFramerFeature *out, uint64_t capacity, uint64_t *count) {
    if (!v || !count) return ADDER_E_BAD_PARAMS;
    *count = v->feat_host.size();
    if (*count > capacity || (*count && !out))
        return vfail(v, ADDER_E_OUT_CAPACITY, "%llu features, room for %llu", (unsigned long long)*count,
                     (unsigned long long)capacity);
    if (*count) memcpy(out, v->feat_host.data(), (size_t)*count * sizeof(AdderFramerFeature));
    return ADDER_OK;
}

extern "C" int adder_viz_player_frame_features(AdderVizPlayer *v, uint64_t *end_ts, uint64_t *offsets, uint16_t *xy,
                                               uint64_t xy_capacity, uint64_t *n_pairs) {
    if (!v || !n_pairs) return ADDER_E_BAD_PARAMS;
    const size_t frames = v->fi_end.size();
    if (!offsets || (frames && !end_ts)) return vfail(v, ADDER_E_BAD_PARAMS, "null offsets / end_ts");
    *n_pairs = v->fi_xy.size() / 2u;
    if (*n_pairs > xy_capacity || (*n_pairs && !xy))
        return vfail(v, ADDER_E_OUT_CAPACITY, "%llu features in the frames' intervals, room for %llu",
                     (unsigned long long)*n_pairs, (unsigned long long)xy_capacity);
    if (frames) memcpy(end_ts, v->fi_end.data(), frames * sizeof(uint64_t));
    memcpy(offsets, v->fi_off.data(), (frames + 1u) * sizeof(uint64_t));
    if (*n_pairs) memcpy(xy, v->fi_xy.data(), v->fi_xy.size() * sizeof(uint16_t));
    if (v->intervals.broken) return vfail(v, ADDER_E_BAD_PARAMS, "%s", v->intervals.err.c_str());
    return ADDER_OK;
}

extern "C" int adder_viz_player_running_intensities(AdderVizPlayer *v, uint8_t *out) {
    if (!v || !out) return ADDER_E_BAD_PARAMS;
    if (!v->plane) {  // detection was never on
        memset(out, 0, v->a.units);
        return ADDER_OK;
    }
    VHIPCHK(v, hipSetDevice(v->p.device_id));
    VHIPCHK(v, hipMemcpyAsync(out, v->plane, v->a.units, hipMemcpyDeviceToHost, v->stream));
    VHIPCHK(v, hipStreamSynchronize(v->stream));
    return ADDER_OK;
}

extern "C" int adder_viz_player_running_intensities_device(AdderVizPlayer *v, uint8_t *d_out, void *stream) {
    if (!v || !d_out) return ADDER_E_BAD_PARAMS;
    VHIPCHK(v, hipSetDevice(v->p.device_id));
    if (!v->plane) {
        VHIPCHK(v, hipMemsetAsync(d_out, 0, v->a.units, (hipStream_t)stream));
        return ADDER_OK;
    }
    VHIPCHK(v, hipMemcpyAsync(d_out, v->plane, v->a.units, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return ADDER_OK;
}

// The three places where the pop schedule meets detection, on the host (self-tests): the functions the kernels run.
// mark_out[i] = mark[i] unless event i is the first of a period; w_out[i] = w0 + the pops before event i.
extern "C" int adder_viz_features_host(const int32_t *pops, uint32_t n_pops, uint64_t n, const uint8_t *mark, int32_t w0,
                                       uint8_t *mark_out, int32_t *w_out) {
    if ((n_pops && !pops) || (n && (!mark || !mark_out || !w_out))) return ADDER_E_BAD_PARAMS;
    for (uint32_t k = 1; k < n_pops; ++k)
        if (pops[k] < pops[k - 1]) return ADDER_E_BAD_PARAMS;
    for (uint64_t i = 0; i < n; ++i) {
        mark_out[i] = (mark[i] != 0u && !viz_period_start(pops, n_pops, (int64_t)i)) ? 1u : 0u;
        w_out[i] = w0 + (int32_t)viz_pops_before(pops, n_pops, (int64_t)i);
    }
    return ADDER_OK;
}

// The hand-out's running frame: some / val are [n_pops][units] (the popped frames), stamps the sorted viz_stamp_key
// list; running is read and left as the context's running frame would be, frames receives the RUNNING form.
extern "C" int adder_viz_overlay_host(uint32_t units, uint32_t n_pops, const uint8_t *some, const uint8_t *val,
                                      const uint64_t *stamps, uint32_t n_stamps, uint8_t *running, uint8_t *frames) {
    if (!running || (n_pops && (!some || !val || !frames)) || (n_stamps && !stamps)) return ADDER_E_BAD_PARAMS;
    for (uint32_t q = 1; q < n_stamps; ++q)
        if (stamps[q] < stamps[q - 1]) return ADDER_E_BAD_PARAMS;
    const unsigned long long *st = reinterpret_cast<const unsigned long long *>(stamps);
    for (uint32_t u = 0; u < units; ++u) {
        uint32_t q = viz_stamp_first(st, n_stamps, u), cur = running[u];
        for (uint32_t k = 0; k < n_pops; ++k) {
            const size_t at = (size_t)k * units + u;
            cur = viz_running_step(cur, some[at] != 0u, val[at], viz_stamp_take(st, n_stamps, q, u, k));
            frames[at] = (uint8_t)cur;
        }
        running[u] = (uint8_t)cur;
    }
    return ADDER_OK;
}

// The schedule on the host (self-tests): the call-level arrays built in plain loops, then viz_schedule with rows in a
// loop -- the function the schedule kernel runs with a block reduction.
extern "C" int64_t adder_viz_schedule_host(const int32_t *row, const int32_t *from, const int32_t *to, const int32_t *L,
                                           uint64_t n, uint32_t rows, uint32_t row_units, int has_limit, uint32_t limit,
                                           int finish, int64_t *pop_index, uint8_t *flushed, uint64_t cap) {
    if (!rows || !row_units || (has_limit && !limit) || n > (1u << 24) || (n && (!row || !from || !to || !L))) return -1;
    int32_t max_l = -1;
    for (uint64_t i = 0; i < n; ++i) {
        if (row[i] < 0 || (uint32_t)row[i] >= rows || to[i] < from[i] || from[i] < -1 || to[i] > (1 << 20)) return -1;
        max_l = std::max(max_l, std::max(L[i], to[i]));
    }
    const uint32_t ring = (uint32_t)max_l + 2u;
    const size_t cells = (size_t)rows * ring;
    std::vector<uint32_t> cnt_carry(cells, 0u), cnt_call(cells, 0u), ridx(n);
    std::vector<int32_t> nat_call(cells, -1), pm(n);
    std::vector<uint8_t> done_carry(rows, 0u), done(rows, 0u), fl((size_t)ring + 1u);
    std::vector<int32_t> pops((size_t)ring + 1u);
    std::vector<unsigned long long> comb(n);
    for (uint64_t i = 0; i < n; ++i) {
        for (int32_t f = from[i] + 1; f <= to[i]; ++f) {
            const size_t at = (size_t)row[i] * ring + (size_t)f % ring;
            cnt_call[at] += 1u;
            nat_call[at] = std::max(nat_call[at], (int32_t)i);
        }
        pm[i] = std::max(i ? pm[i - 1] : -1, L[i]);
    }
    std::iota(ridx.begin(), ridx.end(), 0u);
    std::stable_sort(ridx.begin(), ridx.end(), [&](uint32_t x, uint32_t y) { return row[x] < row[y]; });
    unsigned long long run = 0;
    for (uint64_t p = 0; p < n; ++p) {
        const unsigned long long c = ((unsigned long long)row[ridx[p]] << 32) | (unsigned long long)(uint32_t)(L[ridx[p]] + 1);
        run = std::max(run, c);
        comb[p] = run;
    }
    VizSchedIn v{};
    v.n = (int64_t)n;
    v.n_all = (int64_t)n;
    v.comb = comb.data();
    v.ridx = ridx.data();
    v.pm = pm.data();
    v.cnt_carry = cnt_carry.data();
    v.cnt_call = cnt_call.data();
    v.nat_call = nat_call.data();
    v.done_carry = done_carry.data();
    v.rows = rows;
    v.row_units = row_units;
    v.ring = ring;
    v.w0 = 0;
    v.m0 = -1;
    v.has_limit = has_limit ? 1 : 0;
    v.limit = limit;
    v.opening = 0;
    v.finish = finish;
    v.max_pops = ring + 1u;
    VizSchedOut o{};
    o.pops = pops.data();
    o.flushed = fl.data();
    o.done = done.data();
    VizSerialRows red{rows};
    viz_schedule(v, red, o);
    if (o.overflow || o.n_pops > cap) return -1;
    for (uint32_t k = 0; k < o.n_pops; ++k) {
        if (pop_index) pop_index[k] = pops[k];
        if (flushed) flushed[k] = fl[k];
    }
    return (int64_t)o.n_pops;
}
