// adder_player_api.cpp -- C-ABI of the latest-event player (include/adder_player.h): header parsing, the per-unit
// state and call scratch in HBM, the launches of adder_player.hip and the clock, which lives on the host (every call
// waits for its stream anyway).  No CPU fallback.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <new>

#include "../../include/adder_player.h"
#include "adder_api_util.hpp"
#include "adder_player_kernels.h"
#include "adder_player_logic.hpp"
#include "adder_wire.hpp"

using namespace adder;

static thread_local std::string g_player_create_error;

struct AdderPlayer {
    AdderPlayerParams p{};
    PlayerArgs a{};
    uint32_t current_t = 0;
    uint64_t frame_count = 1;
    hipStream_t stream = nullptr;  // the host-pointer forms' stream
    uint64_t cap = 0;              // call scratch, for `cap` events
    PlayerScratch s{};
    PlayerScalars *h_sc = nullptr;  // pinned
    void *d_in = nullptr;           // host-pointer forms: the input and the frames on the device
    size_t d_in_cap = 0;
    void *d_out = nullptr;
    size_t d_out_cap = 0;
    std::string err;
};

static int pfail(AdderPlayer *v, int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    api_fail(v ? v->err : g_player_create_error, code, fmt, ap);
    va_end(ap);
    return code;
}

#define PHIPCHK(v, expr) ADDER_HIPCHK(pfail, v, expr, #expr)

static size_t elem_bytes(const AdderPlayer *v) { return v->p.out_type == ADDER_PLAYER_U8 ? 1u : 8u; }
static size_t frame_bytes(const AdderPlayer *v) { return (size_t)v->a.units * elem_bytes(v); }

static void free_scratch(AdderPlayer *v) {
    api_free_all({v->s.keys0, v->s.keys1, v->s.idx0, v->s.idx1, v->s.s_val, v->s.s_ts, v->s.cand, v->s.cur, v->s.term,
                  v->s.pmin, v->s.mark, v->s.offs, v->s.pos, v->s.temp});
    PlayerScalars *sc = v->s.sc;
    v->s = PlayerScratch{};
    v->s.sc = sc;
    v->cap = 0;
}

static void player_free(AdderPlayer *v) {
    if (!v) return;
    (void)hipSetDevice(v->p.device_id);
    if (v->stream) (void)hipStreamSynchronize(v->stream);
    (void)hipDeviceSynchronize();
    free_scratch(v);
    api_free_all({v->a.last_ts, v->a.display, v->a.run_lo, v->s.sc, v->d_in, v->d_out});
    if (v->h_sc) (void)hipHostFree(v->h_sc);
    if (v->stream) (void)hipStreamDestroy(v->stream);
    delete v;
}

static int ensure_scratch(AdderPlayer *v, uint64_t n) {
    if (n <= v->cap && v->cap > 0) return ADDER_OK;
    free_scratch(v);
    uint64_t c = n + n / 8u + 1u;
    if (c > (uint64_t)INT32_MAX - 1u) c = (uint64_t)INT32_MAX - 1u;
    const uint64_t m = c + 1u;
    PHIPCHK(v, hipMalloc((void **)&v->s.keys0, c * 4u));
    PHIPCHK(v, hipMalloc((void **)&v->s.keys1, c * 4u));
    PHIPCHK(v, hipMalloc((void **)&v->s.idx0, c * 4u));
    PHIPCHK(v, hipMalloc((void **)&v->s.idx1, c * 4u));
    PHIPCHK(v, hipMalloc((void **)&v->s.s_val, c * 8u));
    PHIPCHK(v, hipMalloc((void **)&v->s.s_ts, c * 4u));
    PHIPCHK(v, hipMalloc((void **)&v->s.cand, m * 4u));
    PHIPCHK(v, hipMalloc((void **)&v->s.cur, m * 4u));
    PHIPCHK(v, hipMalloc((void **)&v->s.term, m * 8u));
    PHIPCHK(v, hipMalloc((void **)&v->s.pmin, m * 8u));
    PHIPCHK(v, hipMalloc((void **)&v->s.mark, m));
    PHIPCHK(v, hipMalloc((void **)&v->s.offs, m * 4u));
    PHIPCHK(v, hipMalloc((void **)&v->s.pos, m * 4u));
    v->s.temp_bytes = player_temp_bytes(c);
    PHIPCHK(v, hipMalloc(&v->s.temp, v->s.temp_bytes));
    v->cap = c;
    return ADDER_OK;
}

extern "C" int adder_player_parse_header(const uint8_t *b, size_t len, AdderPlayerParams *p, uint32_t *header_bytes,
                                         uint32_t *event_bytes) {
    RawHeader h;
    if (!p || !raw_header_parse(b, len, &h) || !raw_header_events_ok(h)) return ADDER_E_BAD_PARAMS;
    AdderPlayerParams q{};
    q.abi_version = ADDER_PLAYER_ABI_VERSION;
    q.width = (uint16_t)h.width;
    q.height = (uint16_t)h.height;
    q.tps = h.tps;
    q.ref_interval = h.ref_interval;
    q.channels = (uint8_t)h.channels;
    q.source_camera = h.source_camera;
    q.time_mode = (uint8_t)h.time_mode;  // the low byte, whatever it says: adder_player_create reads 1 as AbsoluteT
    q.playback_fps = 60.0;
    q.out_type = ADDER_PLAYER_F64;
    q.device_id = 0;
    *p = q;
    if (header_bytes) *header_bytes = h.header_bytes;
    if (event_bytes) *event_bytes = h.event_size;
    return ADDER_OK;
}

extern "C" int adder_player_create(const AdderPlayerParams *p, AdderPlayer **out) {
    if (!p || !out) return pfail(nullptr, ADDER_E_BAD_PARAMS, "null argument");
    *out = nullptr;
    if (p->abi_version != ADDER_PLAYER_ABI_VERSION)
        return pfail(nullptr, ADDER_E_BAD_PARAMS, "abi_version %u, this library is %u", p->abi_version,
                     ADDER_PLAYER_ABI_VERSION);
    if (p->width == 0 || p->height == 0 || (p->channels != 1 && p->channels != 3))
        return pfail(nullptr, ADDER_E_BAD_PARAMS, "plane %ux%ux%u", p->width, p->height, p->channels);
    if (p->ref_interval == 0) return pfail(nullptr, ADDER_E_BAD_PARAMS, "ref_interval must be > 0");
    if (!std::isfinite(p->playback_fps) || !(p->playback_fps > 0.0))
        return pfail(nullptr, ADDER_E_BAD_PARAMS, "playback_fps %g must be finite and positive", p->playback_fps);
    if (player_max_intensity(p->source_camera) == 0.0)
        return pfail(nullptr, ADDER_E_BAD_PARAMS, "source camera %u: the reference's player has no scaling for it",
                     p->source_camera);
    if (p->out_type != ADDER_PLAYER_F64 && p->out_type != ADDER_PLAYER_U8)
        return pfail(nullptr, ADDER_E_BAD_PARAMS, "out_type %d", p->out_type);
    if (const int rc = api_check_device(p->device_id, g_player_create_error)) return rc;
    AdderPlayer *v = new (std::nothrow) AdderPlayer();
    if (!v) return pfail(nullptr, ADDER_E_BAD_PARAMS, "out of host memory");
    v->p = *p;
    PlayerArgs &a = v->a;
    a.width = p->width;
    a.height = p->height;
    a.channels = p->channels;
    a.units = (uint32_t)p->width * p->height * p->channels;
    a.key_bits = key_bits_for(a.units);  // keys 0..units (units: takes part in nothing)
    a.absolute = p->time_mode == ADDER_TIME_ABSOLUTE_T ? 1u : 0u;
    a.ref = p->ref_interval;
    a.out_type = p->out_type;
    a.ref_f = (double)p->ref_interval;
    a.m = player_max_intensity(p->source_camera);
    a.fl = player_frame_length(p->tps, p->playback_fps);
    const size_t u = a.units;
    int rc = ADDER_OK;
    auto mk = [&](void **b, size_t bytes) {
        if (rc == ADDER_OK && hipMalloc(b, bytes) != hipSuccess) rc = ADDER_E_HIP;
    };
    if (hipSetDevice(p->device_id) != hipSuccess) rc = ADDER_E_HIP;
    mk((void **)&a.last_ts, u * 4u);
    mk((void **)&a.display, u * 8u);
    mk((void **)&a.run_lo, (u + 1u) * 4u);
    mk((void **)&v->s.sc, sizeof(PlayerScalars));
    if (rc == ADDER_OK && hipHostMalloc((void **)&v->h_sc, sizeof(PlayerScalars), hipHostMallocDefault) != hipSuccess)
        rc = ADDER_E_HIP;
    if (rc == ADDER_OK && hipStreamCreateWithFlags(&v->stream, hipStreamNonBlocking) != hipSuccess) rc = ADDER_E_HIP;
    if (rc == ADDER_OK && hipMemset(a.last_ts, 0, u * 4u) != hipSuccess) rc = ADDER_E_HIP;
    if (rc == ADDER_OK && hipMemset(a.display, 0, u * 8u) != hipSuccess) rc = ADDER_E_HIP;
    if (rc == ADDER_OK && hipDeviceSynchronize() != hipSuccess) rc = ADDER_E_HIP;  // the calls run on other streams
    if (rc != ADDER_OK) {
        player_free(v);
        return pfail(nullptr, rc, "device allocation for %zu units failed", u);
    }
    *out = v;
    return ADDER_OK;
}

extern "C" void adder_player_destroy(AdderPlayer *v) { player_free(v); }

extern "C" int adder_player_reset(AdderPlayer *v) {
    if (!v) return ADDER_E_BAD_PARAMS;
    PHIPCHK(v, hipSetDevice(v->p.device_id));
    PHIPCHK(v, hipDeviceSynchronize());
    PHIPCHK(v, hipMemset(v->a.last_ts, 0, (size_t)v->a.units * 4u));
    PHIPCHK(v, hipMemset(v->a.display, 0, (size_t)v->a.units * 8u));
    PHIPCHK(v, hipDeviceSynchronize());
    v->current_t = 0;
    v->frame_count = 1;
    return ADDER_OK;
}

extern "C" const char *adder_player_last_error(const AdderPlayer *v) {
    return v ? v->err.c_str() : g_player_create_error.c_str();
}

// One call: the schedule, a wait for the frame count, then the hand-out into d_frames (device) or, when `h_frames`
// is given, into the context's own buffer and from there to the host.
static int play(AdderPlayer *v, int source, const void *d_in, uint64_t n, int final_check, void *d_frames,
                void *h_frames, uint64_t frame_cap, uint64_t *n_frames, uint64_t *bad_index, uint64_t *n_consumed,
                hipStream_t stream) {
    if (!v) return ADDER_E_BAD_PARAMS;
    if (n_frames) *n_frames = 0;
    if (bad_index) *bad_index = ADDER_PLAYER_NO_BAD_EVENT;
    if (n_consumed) *n_consumed = 0;
    if (n > (uint64_t)INT32_MAX - 1u)
        return pfail(v, ADDER_E_BAD_PARAMS, "%llu records in one call (at most 2^31 - 2)", (unsigned long long)n);
    if (n > 0 && !d_in) return pfail(v, ADDER_E_BAD_PARAMS, "null input");
    if (frame_cap > 0 && !d_frames && !h_frames)
        return pfail(v, ADDER_E_BAD_PARAMS, "null frames with capacity %llu", (unsigned long long)frame_cap);
    if (((uintptr_t)d_frames & 7u) != 0u) return pfail(v, ADDER_E_BAD_PARAMS, "frames must be 8-byte aligned");
    if (n == 0 && !final_check) return ADDER_OK;
    PHIPCHK(v, hipSetDevice(v->p.device_id));
    int rc = ensure_scratch(v, n);
    if (rc != ADDER_OK) return rc;
    PHIPCHK(v, player_schedule(v->a, source, d_in, n, final_check, v->current_t, v->frame_count, v->s, stream));
    PHIPCHK(v, hipMemcpyAsync(v->h_sc, v->s.sc, sizeof(PlayerScalars), hipMemcpyDeviceToHost, stream));
    PHIPCHK(v, hipStreamSynchronize(stream));
    const PlayerScalars sc = *v->h_sc;
    const bool bad = sc.bad < sc.eof;
    const uint64_t lim = bad ? sc.bad : sc.eof;
    if (n_frames) *n_frames = sc.total;
    if (sc.total > frame_cap)
        return pfail(v, ADDER_E_OUT_CAPACITY, "%llu frames do not fit in %llu", (unsigned long long)sc.total,
                     (unsigned long long)frame_cap);
    const size_t fb = frame_bytes(v);
    if ((sc.total * (uint64_t)v->a.units + 255u) / 256u > (uint64_t)INT32_MAX)
        return pfail(v, ADDER_E_BAD_PARAMS, "%llu frames in one call: play fewer records at a time",
                     (unsigned long long)sc.total);
    if (h_frames) {
        PHIPCHK(v, api_grow(&v->d_out, &v->d_out_cap, sc.total * fb + 8u));
        d_frames = v->d_out;
    }
    PHIPCHK(v, player_handout(v->a, n, lim, sc.total, d_frames, v->s, stream));
    if (h_frames && sc.total)
        PHIPCHK(v, hipMemcpyAsync(h_frames, d_frames, sc.total * fb, hipMemcpyDeviceToHost, stream));
    PHIPCHK(v, hipStreamSynchronize(stream));
    v->current_t = (uint32_t)sc.cur;
    v->frame_count += sc.total;
    if (n_consumed) *n_consumed = sc.eof;
    if (bad) {
        if (bad_index) *bad_index = sc.bad;
        return pfail(v, ADDER_PLAYER_E_BAD_EVENT, "event %llu of the batch lies outside the %ux%ux%u plane",
                     (unsigned long long)sc.bad, v->a.width, v->a.height, v->a.channels);
    }
    return ADDER_OK;
}

extern "C" int adder_player_play_device(AdderPlayer *v, const AdderEvent *d_events, uint64_t n, void *d_frames,
                                        uint64_t frame_cap, uint64_t *n_frames, uint64_t *bad_index, void *stream) {
    return play(v, kSrcEvents, d_events, n, 0, d_frames, nullptr, frame_cap, n_frames, bad_index, nullptr,
                (hipStream_t)stream);
}

extern "C" int adder_player_play_wire_device(AdderPlayer *v, const uint8_t *d_wire, uint64_t n_records, void *d_frames,
                                             uint64_t frame_cap, uint64_t *n_frames, uint64_t *bad_index,
                                             uint64_t *n_consumed, void *stream) {
    if (!v) return ADDER_E_BAD_PARAMS;
    return play(v, wire_source(v->p.channels), d_wire, n_records, 0, d_frames, nullptr, frame_cap, n_frames, bad_index,
                n_consumed, (hipStream_t)stream);
}

extern "C" int adder_player_finish(AdderPlayer *v, void *d_frames, uint64_t frame_cap, uint64_t *n_frames,
                                   void *stream) {
    return play(v, kSrcEvents, nullptr, 0, 1, d_frames, nullptr, frame_cap, n_frames, nullptr, nullptr,
                (hipStream_t)stream);
}

static int play_host(AdderPlayer *v, int source, const void *in, uint64_t n, void *frames, uint64_t frame_cap,
                     uint64_t *n_frames, uint64_t *bad_index, uint64_t *n_consumed) {
    if (!v) return ADDER_E_BAD_PARAMS;
    if (n > (uint64_t)INT32_MAX - 1u) return pfail(v, ADDER_E_BAD_PARAMS, "too many records in one call");
    if (n > 0 && !in) return pfail(v, ADDER_E_BAD_PARAMS, "null input");
    if (frame_cap > 0 && !frames) return pfail(v, ADDER_E_BAD_PARAMS, "null frames");
    PHIPCHK(v, hipSetDevice(v->p.device_id));
    PHIPCHK(v, api_stage_input(&v->d_in, &v->d_in_cap, in, n * wire_record_bytes(source), v->stream));
    static uint8_t none;  // a non-null host target for a capacity of zero
    return play(v, source, v->d_in, n, 0, nullptr, frames ? frames : &none, frame_cap, n_frames, bad_index, n_consumed,
                v->stream);
}

extern "C" int adder_player_play_host(AdderPlayer *v, const AdderEvent *events, uint64_t n, void *frames,
                                      uint64_t frame_cap, uint64_t *n_frames, uint64_t *bad_index) {
    return play_host(v, kSrcEvents, events, n, frames, frame_cap, n_frames, bad_index, nullptr);
}

extern "C" int adder_player_play_wire_host(AdderPlayer *v, const uint8_t *wire, uint64_t n_records, void *frames,
                                           uint64_t frame_cap, uint64_t *n_frames, uint64_t *bad_index,
                                           uint64_t *n_consumed) {
    if (!v) return ADDER_E_BAD_PARAMS;
    return play_host(v, wire_source(v->p.channels), wire, n_records, frames, frame_cap, n_frames, bad_index, n_consumed);
}

extern "C" int adder_player_display_device(AdderPlayer *v, void *d_frame, void *stream) {
    if (!v) return ADDER_E_BAD_PARAMS;
    if (!d_frame) return pfail(v, ADDER_E_BAD_PARAMS, "null frame");
    PHIPCHK(v, hipSetDevice(v->p.device_id));
    PHIPCHK(v, player_display(v->a, d_frame, (hipStream_t)stream));
    PHIPCHK(v, hipStreamSynchronize((hipStream_t)stream));
    return ADDER_OK;
}

extern "C" int adder_player_display(AdderPlayer *v, void *frame) {
    if (!v) return ADDER_E_BAD_PARAMS;
    if (!frame) return pfail(v, ADDER_E_BAD_PARAMS, "null frame");
    PHIPCHK(v, hipSetDevice(v->p.device_id));
    const size_t fb = frame_bytes(v);
    PHIPCHK(v, api_grow(&v->d_out, &v->d_out_cap, fb + 8u));
    PHIPCHK(v, player_display(v->a, v->d_out, v->stream));
    PHIPCHK(v, hipMemcpyAsync(frame, v->d_out, fb, hipMemcpyDeviceToHost, v->stream));
    PHIPCHK(v, hipStreamSynchronize(v->stream));
    return ADDER_OK;
}

extern "C" int adder_player_clock(const AdderPlayer *v, uint32_t *current_t, uint64_t *frame_count) {
    if (!v) return ADDER_E_BAD_PARAMS;
    if (current_t) *current_t = v->current_t;
    if (frame_count) *frame_count = v->frame_count;
    return ADDER_OK;
}

extern "C" void adder_player_schedule_host(const uint32_t *cur_before, uint64_t n, uint64_t f0, uint64_t fl,
                                           uint8_t *marks) {
    player_schedule_marks(cur_before, n, f0, fl > (1ull << 32) ? (1ull << 32) : fl, marks);
}

extern "C" uint64_t adder_player_frame_length(uint32_t tps, double playback_fps) {
    return player_frame_length(tps, playback_fps);
}
