// adder_dvs_api.cpp -- C-ABI of the ADDER -> DVS conversion (include/adder_dvs.h): header parsing, the per-unit
// state and call scratch in HBM, the launches of adder_dvs.hip, and the host helpers of the .dat / text writer
// (adder-to-dvs/src/main.rs:151-163, 486-554); and of the tool's event video and count map (adder_dvs_video.hip): the
// frame ring and the counts in HBM, the deque's three words of state and the list of frames ready to pop on the host.
// No CPU fallback.
#include <hip/hip_runtime.h>

#include <climits>
#include <new>
#include <vector>

#include "../../include/adder_dvs.h"
#include "adder_api_util.hpp"
#include "adder_dvs_kernels.h"
#include "adder_dvs_video_logic.hpp"
#include "adder_log1p.hpp"
#include "adder_wire.hpp"

using namespace adder;

static thread_local std::string g_dvs_create_error;

struct AdderDvs {
    AdderDvsParams p{};
    DvsArgs a{};
    hipStream_t stream = nullptr;  // the host-pointer forms' stream
    // call scratch, for `cap` events
    uint64_t cap = 0;
    DvsScratch s{};
    DvsScalars *h_sc = nullptr;  // pinned
    // host-pointer forms: the input and output on the device
    void *d_in = nullptr;
    size_t d_in_cap = 0;
    void *d_out = nullptr;
    size_t d_out_cap = 0;
    // sort scratch
    uint64_t sort_cap = 0;
    uint32_t *sk = nullptr;
    void *sort_tmp = nullptr, *sort_temp = nullptr;
    size_t sort_temp_bytes = 0;
    // the event video (adder_dvs_video_enable): its carried state lives here, the frames and counts on the device
    bool video = false, finished = false;
    bool converted = false;         // an event was converted since create / reset
    DvsVideoArgs va{};              // parameters, ring, counts and the call scratch (for `vcap` events)
    uint64_t vcap = 0;
    DvsVideoState vst{0, 0, 1};     // frame_count, current_t, end
    std::vector<uint64_t> ready;    // emitted frames not yet popped, oldest first
    uint64_t ring_needed = 0;
    DvsVideoScalars *h_vs = nullptr;  // pinned
    uint64_t *d_list = nullptr;     // pop: the ready indices on the device
    size_t d_list_cap = 0;
    void *d_pop = nullptr;          // host forms of pop and count map
    size_t d_pop_cap = 0;
    uint32_t *d_m = nullptr;
    std::string err;
};

static int dfail(AdderDvs *v, int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    api_fail(v ? v->err : g_dvs_create_error, code, fmt, ap);
    va_end(ap);
    return code;
}

#define DHIPCHK(v, expr) ADDER_HIPCHK(dfail, v, expr, #expr)

static void free_scratch(AdderDvs *v) {
    api_free_all({v->s.keys0, v->s.keys1, v->s.idx0, v->s.idx1, v->s.s_ln, v->s.s_td, v->s.flag, v->s.tout, v->s.offs,
                  v->s.temp});
    DvsScalars *sc = v->s.sc;
    v->s = DvsScratch{};
    v->s.sc = sc;
    v->cap = 0;
}

static void free_video_scratch(AdderDvs *v) {
    DvsVideoArgs &a = v->va;
    api_free_all({a.pt, a.term, a.reach, a.mark, a.moffs, a.list, a.k0, a.k1, a.v0, a.v1, a.temp});
    a.pt = a.reach = a.list = a.k0 = a.k1 = nullptr;
    a.term = nullptr;
    a.mark = nullptr;
    a.moffs = a.v0 = a.v1 = nullptr;
    a.temp = nullptr;
    a.temp_bytes = 0;
    v->vcap = 0;
}

static void free_video(AdderDvs *v) {
    free_video_scratch(v);
    api_free_all({v->va.ring, v->va.cur_cnt, v->va.nxt_cnt, v->va.vs, v->d_list, v->d_pop, v->d_m});
    if (v->h_vs) (void)hipHostFree(v->h_vs);
    v->va = DvsVideoArgs{};
    v->h_vs = nullptr;
    v->d_list = nullptr;
    v->d_pop = nullptr;
    v->d_m = nullptr;
    v->d_list_cap = v->d_pop_cap = 0;
    v->video = false;
}

static void free_sort(AdderDvs *v) {
    api_free_all({v->sk, v->sort_tmp, v->sort_temp});
    v->sk = nullptr;
    v->sort_tmp = v->sort_temp = nullptr;
    v->sort_cap = 0;
    v->sort_temp_bytes = 0;
}

static void dvs_free(AdderDvs *v) {
    if (!v) return;
    (void)hipSetDevice(v->p.device_id);
    if (v->stream) (void)hipStreamSynchronize(v->stream);
    (void)hipDeviceSynchronize();
    free_scratch(v);
    free_sort(v);
    free_video(v);
    api_free_all({v->a.cur_init, v->a.nxt_init, v->a.cur_ln, v->a.nxt_ln, v->a.cur_t, v->a.nxt_t, v->s.sc, v->d_in,
                  v->d_out});
    if (v->h_sc) (void)hipHostFree(v->h_sc);
    if (v->stream) (void)hipStreamDestroy(v->stream);
    delete v;
}

static int ensure_scratch(AdderDvs *v, uint64_t n) {
    if (n <= v->cap) return ADDER_OK;
    free_scratch(v);
    const uint64_t c = scratch_capacity(n);
    DHIPCHK(v, hipMalloc((void **)&v->s.keys0, c * 4u));
    DHIPCHK(v, hipMalloc((void **)&v->s.keys1, c * 4u));
    DHIPCHK(v, hipMalloc((void **)&v->s.idx0, c * 4u));
    DHIPCHK(v, hipMalloc((void **)&v->s.idx1, c * 4u));
    DHIPCHK(v, hipMalloc((void **)&v->s.s_ln, c * 8u));
    DHIPCHK(v, hipMalloc((void **)&v->s.s_td, c * 8u));
    DHIPCHK(v, hipMalloc((void **)&v->s.flag, c));
    DHIPCHK(v, hipMalloc((void **)&v->s.tout, c * 8u));
    DHIPCHK(v, hipMalloc((void **)&v->s.offs, c * 4u));
    v->s.temp_bytes = dvs_temp_bytes(c);
    DHIPCHK(v, hipMalloc(&v->s.temp, v->s.temp_bytes));
    v->cap = c;
    return ADDER_OK;
}

static int ensure_video_scratch(AdderDvs *v, uint64_t n) {
    if (n <= v->vcap) return ADDER_OK;
    free_video_scratch(v);
    const uint64_t c = scratch_capacity(n);
    DvsVideoArgs &a = v->va;
    DHIPCHK(v, hipMalloc((void **)&a.pt, c * 8u));
    DHIPCHK(v, hipMalloc((void **)&a.term, c * 8u));
    DHIPCHK(v, hipMalloc((void **)&a.reach, c * 8u));
    DHIPCHK(v, hipMalloc((void **)&a.mark, c));
    DHIPCHK(v, hipMalloc((void **)&a.moffs, c * 4u));
    DHIPCHK(v, hipMalloc((void **)&a.list, c * 8u));
    if (a.draw) {
        DHIPCHK(v, hipMalloc((void **)&a.k0, c * 8u));
        DHIPCHK(v, hipMalloc((void **)&a.k1, c * 8u));
        DHIPCHK(v, hipMalloc((void **)&a.v0, c * 4u));
        DHIPCHK(v, hipMalloc((void **)&a.v1, c * 4u));
    }
    a.temp_bytes = dvs_video_temp_bytes(c);
    DHIPCHK(v, hipMalloc(&a.temp, a.temp_bytes));
    v->vcap = c;
    return ADDER_OK;
}

static size_t record_bytes(int fmt) { return fmt == ADDER_DVS_OUT_DAT ? 8u : sizeof(AdderDvsEvent); }

extern "C" int adder_dvs_parse_header(const uint8_t *b, size_t len, AdderDvsParams *p, uint32_t *header_bytes,
                                      uint32_t *event_bytes) {
    RawHeader h;
    if (!p || !raw_header_parse(b, len, &h) || !raw_header_events_ok(h)) return ADDER_E_BAD_PARAMS;
    AdderDvsParams q{};
    q.abi_version = ADDER_DVS_ABI_VERSION;
    q.width = (uint16_t)h.width;
    q.height = (uint16_t)h.height;
    q.ref_interval = h.ref_interval;
    q.channels = (uint8_t)h.channels;
    q.source_camera = h.source_camera;
    q.time_mode = (uint8_t)h.time_mode;  // the low byte, whatever it says: adder_dvs_create reads 0 as DeltaT
    q.theta = 0.01;
    q.device_id = 0;
    *p = q;
    if (header_bytes) *header_bytes = h.header_bytes;
    if (event_bytes) *event_bytes = h.event_size;
    return ADDER_OK;
}

extern "C" int adder_dvs_create(const AdderDvsParams *p, AdderDvs **out) {
    if (!p || !out) return dfail(nullptr, ADDER_E_BAD_PARAMS, "null argument");
    *out = nullptr;
    if (p->abi_version != ADDER_DVS_ABI_VERSION)
        return dfail(nullptr, ADDER_E_BAD_PARAMS, "abi_version %u, this library is %u", p->abi_version,
                     ADDER_DVS_ABI_VERSION);
    if (p->width == 0 || p->height == 0 || (p->channels != 1 && p->channels != 3))
        return dfail(nullptr, ADDER_E_BAD_PARAMS, "plane %ux%ux%u", p->width, p->height, p->channels);
    if (p->ref_interval == 0) return dfail(nullptr, ADDER_E_BAD_PARAMS, "ref_interval must be > 0");
    if (const int rc = api_check_device(p->device_id, g_dvs_create_error)) return rc;
    AdderDvs *v = new (std::nothrow) AdderDvs();
    if (!v) return dfail(nullptr, ADDER_E_BAD_PARAMS, "out of host memory");
    v->p = *p;
    DvsArgs &a = v->a;
    a.width = p->width;
    a.height = p->height;
    a.channels = p->channels;
    a.units = (uint32_t)p->width * p->height * p->channels;
    a.key_bits = key_bits_for(a.units);  // keys 0..units (units: never walked)
    a.delta_t = p->time_mode == 0 ? 1u : 0u;
    a.framed = p->source_camera <= 5u ? 1u : 0u;  // is_framed (lib.rs:50-60): FramedU8 .. FramedF64
    a.ref = p->ref_interval;
    a.ref_f = (double)p->ref_interval;
    a.win_hi = dvs_log1p(1.0) - p->theta;
    a.win_lo = dvs_log1p(0.0) + p->theta;
    a.half = p->theta / 2.0;
    const size_t u = a.units;
    int rc = ADDER_OK;
    auto mk = [&](void **b, size_t bytes) {
        if (rc == ADDER_OK && hipMalloc(b, bytes) != hipSuccess) rc = ADDER_E_HIP;
    };
    if (hipSetDevice(p->device_id) != hipSuccess) rc = ADDER_E_HIP;
    mk((void **)&a.cur_init, u);
    mk((void **)&a.nxt_init, u);
    mk((void **)&a.cur_ln, u * 8u);
    mk((void **)&a.nxt_ln, u * 8u);
    mk((void **)&a.cur_t, u * 8u);
    mk((void **)&a.nxt_t, u * 8u);
    mk((void **)&v->s.sc, sizeof(DvsScalars));
    if (rc == ADDER_OK && hipHostMalloc((void **)&v->h_sc, sizeof(DvsScalars), hipHostMallocDefault) != hipSuccess)
        rc = ADDER_E_HIP;
    if (rc == ADDER_OK && hipStreamCreateWithFlags(&v->stream, hipStreamNonBlocking) != hipSuccess) rc = ADDER_E_HIP;
    if (rc == ADDER_OK && hipMemset(a.cur_init, 0, u) != hipSuccess) rc = ADDER_E_HIP;
    if (rc != ADDER_OK) {
        dvs_free(v);
        return dfail(nullptr, rc, "device allocation for %zu units failed", u);
    }
    *out = v;
    return ADDER_OK;
}

extern "C" void adder_dvs_destroy(AdderDvs *v) { dvs_free(v); }

extern "C" int adder_dvs_reset(AdderDvs *v) {
    if (!v) return ADDER_E_BAD_PARAMS;
    DHIPCHK(v, hipSetDevice(v->p.device_id));
    DHIPCHK(v, hipDeviceSynchronize());
    DHIPCHK(v, hipMemset(v->a.cur_init, 0, v->a.units));
    v->converted = false;
    if (v->video) {
        const size_t plane = (size_t)v->a.width * v->a.height;
        DHIPCHK(v, hipMemset(v->va.ring, 128, v->va.ring_frames * plane));
        DHIPCHK(v, hipMemset(v->va.cur_cnt, 0, (size_t)v->a.units * 4u));
        v->vst = DvsVideoState{0, 0, 1};
        v->ready.clear();
        v->ring_needed = 0;
        v->finished = false;
    }
    return ADDER_OK;
}

extern "C" const char *adder_dvs_last_error(const AdderDvs *v) {
    return v ? v->err.c_str() : g_dvs_create_error.c_str();
}

static int convert(AdderDvs *v, int source, const void *d_in, uint64_t n, int fmt, void *d_out, uint64_t out_cap,
                   uint64_t *n_out, uint64_t *bad_index, uint64_t *n_consumed, hipStream_t stream) {
    if (!v) return ADDER_E_BAD_PARAMS;
    if (n_out) *n_out = 0;
    if (bad_index) *bad_index = ADDER_DVS_NO_BAD_EVENT;
    if (n_consumed) *n_consumed = 0;
    if (fmt != ADDER_DVS_OUT_EVENTS && fmt != ADDER_DVS_OUT_DAT)
        return dfail(v, ADDER_E_BAD_PARAMS, "output format %d", fmt);
    if (n > (uint64_t)INT32_MAX) return dfail(v, ADDER_E_BAD_PARAMS, "%llu events in one call (at most 2^31 - 1)",
                                              (unsigned long long)n);
    if (n > 0 && !d_in) return dfail(v, ADDER_E_BAD_PARAMS, "null input");
    if (out_cap > 0 && !d_out) return dfail(v, ADDER_E_BAD_PARAMS, "null output with capacity %llu",
                                            (unsigned long long)out_cap);
    if (v->finished) return dfail(v, ADDER_E_BAD_PARAMS, "the video is finished: reset before converting again");
    if (n == 0) return ADDER_OK;
    DHIPCHK(v, hipSetDevice(v->p.device_id));
    int rc = ensure_scratch(v, n);
    if (rc != ADDER_OK) return rc;
    if (v->video) {
        if ((rc = ensure_video_scratch(v, n)) != ADDER_OK) return rc;
        DvsVideoArgs &va = v->va;
        va.F0 = v->vst.F;
        va.cur0 = v->vst.cur;
        va.E0 = v->vst.E;
        va.lo = v->ready.empty() ? v->vst.F : v->ready.front();
    }
    DHIPCHK(v, dvs_convert(v->a, source, d_in, n, fmt, d_out, out_cap, v->s, stream, v->video ? &v->va : nullptr));
    DHIPCHK(v, hipMemcpyAsync(v->h_sc, v->s.sc, sizeof(DvsScalars), hipMemcpyDeviceToHost, stream));
    if (v->video)
        DHIPCHK(v, hipMemcpyAsync(v->h_vs, v->va.vs, sizeof(DvsVideoScalars), hipMemcpyDeviceToHost, stream));
    DHIPCHK(v, hipStreamSynchronize(stream));
    const DvsScalars sc = *v->h_sc;
    if (n_out) *n_out = sc.total;
    if (n_consumed) *n_consumed = sc.eof;
    const bool bad = sc.bad < sc.eof;
    if (bad && bad_index) *bad_index = sc.bad;
    if (v->video) v->ring_needed = v->h_vs->need;  // of this call, whichever way it ends
    if (sc.total > out_cap)
        return dfail(v, ADDER_E_OUT_CAPACITY, "%llu DVS events do not fit in %llu", (unsigned long long)sc.total,
                     (unsigned long long)out_cap);
    if (v->video) {
        const DvsVideoScalars vs = *v->h_vs;
        if (!vs.ok)
            return dfail(v, ADDER_E_OUT_CAPACITY, "the call needs %llu ring frames, the ring has %llu",
                         (unsigned long long)vs.need, (unsigned long long)v->va.ring_frames);
        if (vs.n_emit) {
            const size_t at = v->ready.size();
            v->ready.resize(at + vs.n_emit);
            DHIPCHK(v, hipMemcpy(v->ready.data() + at, v->va.list, vs.n_emit * 8u, hipMemcpyDeviceToHost));
        }
        v->vst = DvsVideoState{vs.F, vs.cur, vs.E};
    }
    v->converted = true;
    if (bad) {
        return dfail(v, ADDER_DVS_E_BAD_EVENT, "event %llu of the batch cannot be converted (first event of a unit "
                     "with d > 128, d in 129..254, or outside the plane)", (unsigned long long)sc.bad);
    }
    return ADDER_OK;
}

extern "C" int adder_dvs_convert_device(AdderDvs *v, const AdderEvent *d_events, uint64_t n, int fmt, void *d_out,
                                        uint64_t out_cap, uint64_t *n_out, uint64_t *bad_index, void *stream) {
    return convert(v, kSrcEvents, d_events, n, fmt, d_out, out_cap, n_out, bad_index, nullptr, (hipStream_t)stream);
}

extern "C" int adder_dvs_convert_wire_device(AdderDvs *v, const uint8_t *d_wire, uint64_t n_records, int fmt,
                                             void *d_out, uint64_t out_cap, uint64_t *n_out, uint64_t *bad_index,
                                             uint64_t *n_consumed, void *stream) {
    if (!v) return ADDER_E_BAD_PARAMS;
    return convert(v, wire_source(v->p.channels), d_wire, n_records, fmt, d_out, out_cap, n_out, bad_index, n_consumed,
                   (hipStream_t)stream);
}

static int convert_host(AdderDvs *v, int source, const void *in, uint64_t n, int fmt, void *out, uint64_t out_cap,
                        uint64_t *n_out, uint64_t *bad_index, uint64_t *n_consumed) {
    if (!v) return ADDER_E_BAD_PARAMS;
    if (n > (uint64_t)INT32_MAX) return dfail(v, ADDER_E_BAD_PARAMS, "too many events in one call");
    if (n > 0 && !in) return dfail(v, ADDER_E_BAD_PARAMS, "null input");
    if (out_cap > 0 && !out) return dfail(v, ADDER_E_BAD_PARAMS, "null output");
    DHIPCHK(v, hipSetDevice(v->p.device_id));
    const size_t rb = record_bytes(fmt);
    const uint64_t dcap = out_cap < n ? out_cap : n;  // an input event fires at most once
    DHIPCHK(v, api_grow(&v->d_out, &v->d_out_cap, dcap * rb + 1u));
    DHIPCHK(v, api_stage_input(&v->d_in, &v->d_in_cap, in, n * wire_record_bytes(source), v->stream));
    uint64_t got = 0;
    const int rc = convert(v, source, v->d_in, n, fmt, v->d_out, dcap, &got, bad_index, n_consumed, v->stream);
    if (n_out) *n_out = got;
    if ((rc == ADDER_OK || rc == ADDER_DVS_E_BAD_EVENT) && got)
        DHIPCHK(v, hipMemcpy(out, v->d_out, got * rb, hipMemcpyDeviceToHost));
    return rc;
}

extern "C" int adder_dvs_convert_host(AdderDvs *v, const AdderEvent *events, uint64_t n, int fmt, void *out,
                                      uint64_t out_cap, uint64_t *n_out, uint64_t *bad_index) {
    return convert_host(v, kSrcEvents, events, n, fmt, out, out_cap, n_out, bad_index, nullptr);
}

extern "C" int adder_dvs_convert_wire_host(AdderDvs *v, const uint8_t *wire, uint64_t n_records, int fmt, void *out,
                                           uint64_t out_cap, uint64_t *n_out, uint64_t *bad_index,
                                           uint64_t *n_consumed) {
    if (!v) return ADDER_E_BAD_PARAMS;
    return convert_host(v, wire_source(v->p.channels), wire, n_records, fmt, out, out_cap, n_out, bad_index,
                        n_consumed);
}

extern "C" int adder_dvs_sort_device(AdderDvs *v, void *d_records, uint64_t n, int fmt, void *stream) {
    if (!v) return ADDER_E_BAD_PARAMS;
    if (fmt != ADDER_DVS_OUT_EVENTS && fmt != ADDER_DVS_OUT_DAT)
        return dfail(v, ADDER_E_BAD_PARAMS, "output format %d", fmt);
    if (n > (uint64_t)INT32_MAX) return dfail(v, ADDER_E_BAD_PARAMS, "too many records to sort in one call");
    if (n < 2) return ADDER_OK;
    if (!d_records) return dfail(v, ADDER_E_BAD_PARAMS, "null records");
    DHIPCHK(v, hipSetDevice(v->p.device_id));
    if (n > v->sort_cap) {
        free_sort(v);
        DHIPCHK(v, hipMalloc((void **)&v->sk, n * 16u));  // keys0, keys1, vals0, vals1
        DHIPCHK(v, hipMalloc(&v->sort_tmp, n * sizeof(AdderDvsEvent)));
        v->sort_temp_bytes = dvs_sort_temp_bytes(n);
        DHIPCHK(v, hipMalloc(&v->sort_temp, v->sort_temp_bytes));
        v->sort_cap = n;
    }
    const hipStream_t s = (hipStream_t)stream;
    DHIPCHK(v, dvs_sort(d_records, n, fmt, v->sk, v->sk + n, v->sk + 2 * n, v->sk + 3 * n, v->sort_tmp, v->sort_temp,
                        v->sort_temp_bytes, s));
    DHIPCHK(v, hipStreamSynchronize(s));
    return ADDER_OK;
}

extern "C" size_t adder_dvs_header_bytes(uint16_t width, uint16_t height, const char *date, int binary, char *out,
                                         size_t cap) {
    std::string h = "% Height " + std::to_string(height) + "\n% Width " + std::to_string(width) +
                    "\n% Version 2\n% Date " + std::string(date ? date : "") + "\n% end\n";
    if (binary) h += std::string("\x00\x08", 2);
    if (out && h.size() <= cap) memcpy(out, h.data(), h.size());
    return h.size();
}

extern "C" size_t adder_dvs_format_text(const AdderDvsEvent *ev, uint64_t n, char *out, size_t cap) {
    size_t pos = 0;
    char line[64];
    for (uint64_t i = 0; i < n; ++i) {
        const int k = snprintf(line, sizeof line, "%llu %u %u %u\n", (unsigned long long)ev[i].t, (unsigned)ev[i].x,
                               (unsigned)ev[i].y, ev[i].p ? 1u : 0u);
        if (out && pos + (size_t)k <= cap) memcpy(out + pos, line, (size_t)k);
        pos += (size_t)k;
    }
    return pos;
}

extern "C" double adder_dvs_log1p(double x) { return dvs_log1p(x); }

extern "C" void adder_dvs_log1p_host(const double *x, double *y, uint64_t n) {
    for (uint64_t i = 0; i < n; ++i) y[i] = dvs_log1p(x[i]);
}

extern "C" int adder_dvs_log1p_device(const double *d_x, double *d_y, uint64_t n, int device_id) {
    if (hipSetDevice(device_id) != hipSuccess) return ADDER_E_NO_DEVICE;
    if (dvs_log1p_run(d_x, d_y, n, nullptr) != hipSuccess) return ADDER_E_HIP;
    return hipDeviceSynchronize() == hipSuccess ? ADDER_OK : ADDER_E_HIP;
}

// ---- the event video and the count map ----

extern "C" int adder_dvs_video_params_from_header(const uint8_t *b, size_t len, AdderDvsVideoParams *p) {
    RawHeader h;
    if (!p || !raw_header_parse(b, len, &h) || !raw_header_events_ok(h)) return ADDER_E_BAD_PARAMS;
    AdderDvsVideoParams q{};
    q.abi_version = ADDER_DVS_ABI_VERSION;
    q.tps = h.tps;
    q.fps = 100.0f;
    q.buffer_secs = 10.0f;
    q.ring_frames = 0;
    q.draw = 1;
    *p = q;
    return ADDER_OK;
}

extern "C" int adder_dvs_video_params_check(const AdderDvsVideoParams *p, uint64_t *L, uint64_t *B) {
    if (!p || p->abi_version != ADDER_DVS_ABI_VERSION) return ADDER_E_BAD_PARAMS;
    if (!(p->fps > 0.0f) || p->fps * 0.0f != 0.0f) return ADDER_E_BAD_PARAMS;  // not positive, NaN, infinite
    const uint64_t fl = dvs_video_frame_length(p->tps, p->fps);
    if (fl == 0) return ADDER_E_BAD_PARAMS;  // the reference would divide by it
    if (L) *L = fl;
    if (B) *B = dvs_video_buffer_ticks(p->tps, p->buffer_secs);
    return ADDER_OK;
}

extern "C" int adder_dvs_video_enable(AdderDvs *v, const AdderDvsVideoParams *p) {
    if (!v) return ADDER_E_BAD_PARAMS;
    if (!p) return dfail(v, ADDER_E_BAD_PARAMS, "null argument");
    if (v->converted) return dfail(v, ADDER_E_BAD_PARAMS, "events were converted already: enable after create or reset");
    uint64_t L = 0, B = 0;
    if (adder_dvs_video_params_check(p, &L, &B) != ADDER_OK)
        return dfail(v, ADDER_E_BAD_PARAMS, "abi_version %u (this library is %u), tps %u, fps %g: fps must be finite "
                     "and positive, a frame at least one tick", p->abi_version, ADDER_DVS_ABI_VERSION, p->tps,
                     (double)p->fps);
    uint64_t ring = p->ring_frames;
    if (ring == 0) ring = B / L + (B % L != 0 ? 1u : 0u) + 64u;
    const size_t plane = (size_t)v->a.width * v->a.height;
    if (ring > (1ull << 32) / plane + 1u)  // the draw's keys and a sane allocation
        return dfail(v, ADDER_E_BAD_PARAMS, "a ring of %llu frames of %zu bytes", (unsigned long long)ring, plane);
    DHIPCHK(v, hipSetDevice(v->p.device_id));
    DHIPCHK(v, hipDeviceSynchronize());
    free_video(v);
    DvsVideoArgs &a = v->va;
    a.L = L;
    a.B = B;
    a.ring_frames = ring;
    a.draw = p->draw ? 1u : 0u;
    DHIPCHK(v, hipMalloc((void **)&a.ring, ring * plane));
    DHIPCHK(v, hipMalloc((void **)&a.cur_cnt, (size_t)v->a.units * 4u));
    DHIPCHK(v, hipMalloc((void **)&a.nxt_cnt, (size_t)v->a.units * 4u));
    DHIPCHK(v, hipMalloc((void **)&a.vs, sizeof(DvsVideoScalars)));
    DHIPCHK(v, hipMalloc((void **)&v->d_m, 4u));
    DHIPCHK(v, hipHostMalloc((void **)&v->h_vs, sizeof(DvsVideoScalars), hipHostMallocDefault));
    DHIPCHK(v, hipMemset(a.ring, 128, ring * plane));
    DHIPCHK(v, hipMemset(a.cur_cnt, 0, (size_t)v->a.units * 4u));
    v->vst = DvsVideoState{0, 0, 1};
    v->ready.clear();
    v->ring_needed = 0;
    v->finished = false;
    v->video = true;
    return ADDER_OK;
}

static int need_video(AdderDvs *v) {
    if (!v) return ADDER_E_BAD_PARAMS;
    if (!v->video) return dfail(v, ADDER_E_BAD_PARAMS, "the video is not enabled (adder_dvs_video_enable)");
    return ADDER_OK;
}

extern "C" int adder_dvs_video_frames_ready(AdderDvs *v, uint64_t *n) {
    if (const int rc = need_video(v)) return rc;
    if (n) *n = v->ready.size();
    return ADDER_OK;
}

extern "C" int adder_dvs_video_ring_needed(AdderDvs *v, uint64_t *n) {
    if (const int rc = need_video(v)) return rc;
    if (n) *n = v->ring_needed;
    return ADDER_OK;
}

extern "C" int adder_dvs_video_finish(AdderDvs *v) {
    if (const int rc = need_video(v)) return rc;
    if (v->finished) return dfail(v, ADDER_E_BAD_PARAMS, "the video is finished already");
    DvsVideoState st = v->vst;
    uint64_t first = 0;
    const uint64_t k = dvs_video_finish(v->va.L, v->va.B, &st, &first);
    const uint64_t lo = v->ready.empty() ? first : v->ready.front();
    const uint64_t need = first + k - lo;  // the blank frame of an empty deque takes a slot too
    v->ring_needed = need;
    if (need > v->va.ring_frames)
        return dfail(v, ADDER_E_OUT_CAPACITY, "the finish needs %llu ring frames, the ring has %llu: pop first",
                     (unsigned long long)need, (unsigned long long)v->va.ring_frames);
    for (uint64_t f = first; f < first + k; ++f) v->ready.push_back(f);
    v->vst = st;
    v->finished = true;
    return ADDER_OK;
}

extern "C" int adder_dvs_video_pop_device(AdderDvs *v, uint8_t *d_out, uint64_t out_cap, uint64_t *frame_index,
                                          uint64_t *n_popped, void *stream) {
    if (const int rc = need_video(v)) return rc;
    const uint64_t k = v->ready.size();
    if (n_popped) *n_popped = k;
    if (k > out_cap)
        return dfail(v, ADDER_E_OUT_CAPACITY, "%llu ready frames do not fit in %llu", (unsigned long long)k,
                     (unsigned long long)out_cap);
    if (k == 0) return ADDER_OK;
    if (!d_out) return dfail(v, ADDER_E_BAD_PARAMS, "null output");
    DHIPCHK(v, hipSetDevice(v->p.device_id));
    const hipStream_t s = (hipStream_t)stream;
    DHIPCHK(v, api_grow((void **)&v->d_list, &v->d_list_cap, k * 8u));
    DHIPCHK(v, hipMemcpyAsync(v->d_list, v->ready.data(), k * 8u, hipMemcpyHostToDevice, s));
    DHIPCHK(v, dvs_video_handout(v->a, v->va, v->d_list, k, d_out, s));
    DHIPCHK(v, hipStreamSynchronize(s));  // `ready` is pageable: the copy above has read it by now
    if (frame_index) memcpy(frame_index, v->ready.data(), k * 8u);
    v->ready.clear();
    return ADDER_OK;
}

extern "C" int adder_dvs_video_pop(AdderDvs *v, uint8_t *out, uint64_t out_cap, uint64_t *frame_index,
                                   uint64_t *n_popped) {
    if (const int rc = need_video(v)) return rc;
    const uint64_t k = v->ready.size();
    if (k > 0 && k <= out_cap && !out) return dfail(v, ADDER_E_BAD_PARAMS, "null output");
    const size_t plane = (size_t)v->a.width * v->a.height;
    DHIPCHK(v, hipSetDevice(v->p.device_id));
    if (k <= out_cap) DHIPCHK(v, api_grow(&v->d_pop, &v->d_pop_cap, k * plane + 1u));
    const int rc = adder_dvs_video_pop_device(v, (uint8_t *)v->d_pop, out_cap, frame_index, n_popped, v->stream);
    if (rc == ADDER_OK && k) DHIPCHK(v, hipMemcpy(out, v->d_pop, k * plane, hipMemcpyDeviceToHost));
    return rc;
}

extern "C" int adder_dvs_event_count_map_device(AdderDvs *v, uint8_t *d_out, void *stream) {
    if (const int rc = need_video(v)) return rc;
    if (!d_out) return dfail(v, ADDER_E_BAD_PARAMS, "null output");
    DHIPCHK(v, hipSetDevice(v->p.device_id));
    DHIPCHK(v, dvs_video_count_map(v->a, v->va.cur_cnt, v->d_m, d_out, (hipStream_t)stream));
    DHIPCHK(v, hipStreamSynchronize((hipStream_t)stream));
    return ADDER_OK;
}

extern "C" int adder_dvs_event_count_map(AdderDvs *v, uint8_t *out) {
    if (const int rc = need_video(v)) return rc;
    if (!out) return dfail(v, ADDER_E_BAD_PARAMS, "null output");
    const size_t bytes = (size_t)v->a.width * v->a.height * 3u;
    DHIPCHK(v, hipSetDevice(v->p.device_id));
    DHIPCHK(v, api_grow(&v->d_pop, &v->d_pop_cap, bytes));
    const int rc = adder_dvs_event_count_map_device(v, (uint8_t *)v->d_pop, v->stream);
    if (rc != ADDER_OK) return rc;
    DHIPCHK(v, hipMemcpy(out, v->d_pop, bytes, hipMemcpyDeviceToHost));
    return ADDER_OK;
}

extern "C" uint64_t adder_dvs_video_frame_length(uint32_t tps, float fps) { return dvs_video_frame_length(tps, fps); }

extern "C" uint64_t adder_dvs_video_buffer_ticks(uint32_t tps, float secs) { return dvs_video_buffer_ticks(tps, secs); }

extern "C" uint8_t adder_dvs_video_count_byte(uint32_t count, uint32_t m) { return dvs_video_count_byte(count, m); }

extern "C" uint64_t adder_dvs_video_schedule_host(const uint64_t *pt, const uint64_t *fire_t, uint64_t n, uint64_t L,
                                                  uint64_t B, int draw, uint64_t *state, uint8_t *pop, uint8_t *accept,
                                                  uint64_t *emitted, uint64_t cap) {
    if (!state || L == 0 || (n && (!pt || !fire_t))) return 0;
    DvsVideoState st{state[0], state[1], state[2]};
    const uint64_t k = dvs_video_schedule(pt, fire_t, n, L, B, draw != 0, &st, pop, accept, emitted, emitted ? cap : 0);
    state[0] = st.F;
    state[1] = st.cur;
    state[2] = st.E;
    return k;
}
