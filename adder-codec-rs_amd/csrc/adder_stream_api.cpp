// adder_stream_api.cpp -- C-ABI of the stream migration and adder-info (include/adder_stream.h): header parsing and
// rewriting, the per-unit time planes and call scratch in HBM, the launches of adder_stream.hip, the fold's carry and
// the report's text (adder-info/src/main.rs:47-66, 134-147).  No CPU fallback.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>
#include <cmath>
#include <new>

#include "../../include/adder_stream.h"
#include "adder_api_util.hpp"
#include "adder_stream_kernels.h"
#include "adder_wire.hpp"

using namespace adder;

static thread_local std::string g_stream_create_error;

struct AdderStream {
    AdderStreamParams p{};
    StreamArgs a{};          // a.state = the migration's plane
    uint64_t *info_t = nullptr;  // adder-info's plane: the unit's last raw t
    int op = kStreamPass;
    bool info_absolute = false;
    hipStream_t stream = nullptr;  // the host-pointer forms' stream
    uint64_t cap = 0, info_cap = 0;
    StreamScratch s{};
    StreamScalars *h_sc = nullptr;  // pinned
    StreamFold *d_fold = nullptr, *h_fold = nullptr;
    StreamFold fold{};  // the fold after the last call
    void *d_in = nullptr, *d_out = nullptr;  // host-pointer forms
    size_t d_in_cap = 0, d_out_cap = 0;
    std::string err;
};

static int sfail(AdderStream *v, int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    api_fail(v ? v->err : g_stream_create_error, code, fmt, ap);
    va_end(ap);
    return code;
}

#define SHIPCHK(v, expr) ADDER_HIPCHK(sfail, v, expr, #expr)

static const StreamFold kEmptyFold = {DBL_MAX, 0ull, 0ull};

static void free_scratch(AdderStream *v) {
    api_free_all({v->s.keys0, v->s.keys1, v->s.idx0, v->s.idx1, v->s.s_t, v->s.s_o, v->s.temp, v->s.dt, v->s.op,
                  v->s.prefix});
    StreamScalars *sc = v->s.sc;
    v->s = StreamScratch{};
    v->s.sc = sc;
    v->cap = v->info_cap = 0;
}

static void stream_free(AdderStream *v) {
    if (!v) return;
    (void)hipSetDevice(v->p.device_id);
    if (v->stream) (void)hipStreamSynchronize(v->stream);
    (void)hipDeviceSynchronize();
    free_scratch(v);
    api_free_all({v->a.state, v->info_t, v->s.sc, v->d_fold, v->d_in, v->d_out});
    if (v->h_sc) (void)hipHostFree(v->h_sc);
    if (v->h_fold) (void)hipHostFree(v->h_fold);
    if (v->stream) (void)hipStreamDestroy(v->stream);
    delete v;
}

// scratch for n events; the fold's arrays (32 bytes an event) only once an info call asks for them
static int ensure_scratch(AdderStream *v, uint64_t n, bool info) {
    if (n <= v->cap && (!info || n <= v->info_cap)) return ADDER_OK;
    const bool had_info = v->info_cap > 0;
    free_scratch(v);
    const uint64_t c = scratch_capacity(n);
    SHIPCHK(v, hipMalloc((void **)&v->s.keys0, c * 4u));
    SHIPCHK(v, hipMalloc((void **)&v->s.keys1, c * 4u));
    SHIPCHK(v, hipMalloc((void **)&v->s.idx0, c * 4u));
    SHIPCHK(v, hipMalloc((void **)&v->s.idx1, c * 4u));
    SHIPCHK(v, hipMalloc((void **)&v->s.s_t, c * 4u));
    SHIPCHK(v, hipMalloc((void **)&v->s.s_o, c * 4u));
    v->s.temp_bytes = stream_temp_bytes(c);
    SHIPCHK(v, hipMalloc(&v->s.temp, v->s.temp_bytes));
    v->cap = c;
    if (info || had_info) {
        SHIPCHK(v, hipMalloc((void **)&v->s.dt, c * 4u));
        SHIPCHK(v, hipMalloc((void **)&v->s.op, c * sizeof(StreamMinOp)));
        SHIPCHK(v, hipMalloc((void **)&v->s.prefix, c * sizeof(StreamMinOp)));
        v->info_cap = c;
    }
    return ADDER_OK;
}

static void wr32(uint8_t *b, uint32_t v) {
    b[0] = (uint8_t)(v >> 24);
    b[1] = (uint8_t)(v >> 16);
    b[2] = (uint8_t)(v >> 8);
    b[3] = (uint8_t)v;
}

extern "C" int adder_stream_parse_header(const uint8_t *b, size_t len, AdderStreamParams *p, uint32_t *header_bytes,
                                         uint32_t *event_bytes) {
    RawHeader h;
    if (!p || !raw_header_parse(b, len, &h) || !raw_header_events_ok(h)) return ADDER_E_BAD_PARAMS;
    if (h.time_mode > 2u) return ADDER_E_BAD_PARAMS;  // this tool rewrites the field: it has to know what it says
    AdderStreamParams q{};
    q.abi_version = ADDER_STREAM_ABI_VERSION;
    q.width = (uint16_t)h.width;
    q.height = (uint16_t)h.height;
    q.tps = h.tps;
    q.ref_interval = h.ref_interval;
    q.delta_t_max = h.delta_t_max;
    q.channels = (uint8_t)h.channels;
    q.codec_version = (uint8_t)h.version;
    q.source_camera = h.source_camera;
    q.time_mode = q.out_time_mode = (uint8_t)h.time_mode;
    q.device_id = 0;
    *p = q;
    if (header_bytes) *header_bytes = h.header_bytes;
    if (event_bytes) *event_bytes = h.event_size;
    return ADDER_OK;
}

extern "C" size_t adder_stream_migrated_header(const uint8_t *in, size_t len, uint32_t time_mode, uint8_t *out,
                                               size_t cap) {
    AdderStreamParams p;
    uint32_t hb = 0;
    if (adder_stream_parse_header(in, len, &p, &hb, nullptr) != ADDER_OK || time_mode > 2u) return 0;
    const uint32_t version = p.codec_version < 2 ? 2u : p.codec_version;
    const size_t n = 25u + 4u * version;
    if (!out || n > cap) return n;
    memcpy(out, in, 25);
    out[5] = (uint8_t)version;
    wr32(out + 25, p.source_camera);
    wr32(out + 29, time_mode);
    if (version >= 3) memcpy(out + 33, in + 33, 4);
    return n;
}

extern "C" int adder_stream_create(const AdderStreamParams *p, AdderStream **out) {
    if (!p || !out) return sfail(nullptr, ADDER_E_BAD_PARAMS, "null argument");
    *out = nullptr;
    if (p->abi_version != ADDER_STREAM_ABI_VERSION)
        return sfail(nullptr, ADDER_E_BAD_PARAMS, "abi_version %u, this library is %u", p->abi_version,
                     ADDER_STREAM_ABI_VERSION);
    if (p->width == 0 || p->height == 0 || (p->channels != 1 && p->channels != 3))
        return sfail(nullptr, ADDER_E_BAD_PARAMS, "plane %ux%ux%u", p->width, p->height, p->channels);
    // keys are 32 bits wide and the sentinel key is `units` itself: units + 1 keys have to fit
    const uint64_t units64 = (uint64_t)p->width * p->height * p->channels;
    if (units64 + 1u > (uint64_t)UINT32_MAX)
        return sfail(nullptr, ADDER_E_BAD_PARAMS, "plane %ux%ux%u: %llu units and the sentinel key do not fit 32 bits",
                     p->width, p->height, p->channels, (unsigned long long)units64);
    if (p->ref_interval == 0) return sfail(nullptr, ADDER_E_BAD_PARAMS, "ref_interval must be > 0");
    if (p->codec_version > 3 || p->time_mode > 2 || p->out_time_mode > 2)
        return sfail(nullptr, ADDER_E_BAD_PARAMS, "codec version %u, time modes %u -> %u", p->codec_version,
                     p->time_mode, p->out_time_mode);
    if (const int rc = api_check_device(p->device_id, g_stream_create_error)) return rc;
    AdderStream *v = new (std::nothrow) AdderStream();
    if (!v) return sfail(nullptr, ADDER_E_BAD_PARAMS, "out of host memory");
    v->p = *p;
    StreamArgs &a = v->a;
    a.width = p->width;
    a.height = p->height;
    a.channels = p->channels;
    a.units = (uint32_t)units64;
    a.key_bits = key_bits_for(a.units);  // keys 0..units (units: never worked on)
    a.ref = p->ref_interval;
    // a v0 / v1 stream has no time-mode field: it is DeltaT
    const uint32_t in_mode = p->codec_version >= 2 ? p->time_mode : (uint32_t)ADDER_TIME_DELTA_T;
    const bool framed = p->source_camera <= 5u;  // is_framed (lib.rs:50-60): FramedU8 .. FramedF64
    if (in_mode == ADDER_TIME_DELTA_T && p->out_time_mode == ADDER_TIME_ABSOLUTE_T) {
        v->op = kStreamForward;
        a.round = framed && p->codec_version > 0 ? 1u : 0u;  // stream_migration.rs:65
    } else if (in_mode == ADDER_TIME_ABSOLUTE_T && p->out_time_mode == ADDER_TIME_DELTA_T) {
        v->op = kStreamInverse;
        a.round = framed ? 1u : 0u;
    } else {
        v->op = kStreamPass;
        a.round = 0u;
    }
    v->info_absolute = p->codec_version >= 2 && p->time_mode == ADDER_TIME_ABSOLUTE_T;  // main.rs:91
    v->fold = kEmptyFold;
    const size_t u = a.units;
    int rc = ADDER_OK;
    auto mk = [&](void **b, size_t bytes) {
        if (rc == ADDER_OK && hipMalloc(b, bytes) != hipSuccess) rc = ADDER_E_HIP;
    };
    if (hipSetDevice(p->device_id) != hipSuccess) rc = ADDER_E_HIP;
    mk((void **)&a.state, u * 8u);
    mk((void **)&v->info_t, u * 8u);
    mk((void **)&v->s.sc, sizeof(StreamScalars));
    mk((void **)&v->d_fold, sizeof(StreamFold));
    if (rc == ADDER_OK && hipHostMalloc((void **)&v->h_sc, sizeof(StreamScalars), hipHostMallocDefault) != hipSuccess)
        rc = ADDER_E_HIP;
    if (rc == ADDER_OK && hipHostMalloc((void **)&v->h_fold, sizeof(StreamFold), hipHostMallocDefault) != hipSuccess)
        rc = ADDER_E_HIP;
    if (rc == ADDER_OK && hipStreamCreateWithFlags(&v->stream, hipStreamNonBlocking) != hipSuccess) rc = ADDER_E_HIP;
    if (rc == ADDER_OK && hipMemset(a.state, 0, u * 8u) != hipSuccess) rc = ADDER_E_HIP;
    if (rc == ADDER_OK && hipMemset(v->info_t, 0, u * 8u) != hipSuccess) rc = ADDER_E_HIP;
    if (rc == ADDER_OK && hipMemcpy(v->d_fold, &kEmptyFold, sizeof kEmptyFold, hipMemcpyHostToDevice) != hipSuccess)
        rc = ADDER_E_HIP;
    if (rc != ADDER_OK) {
        stream_free(v);
        return sfail(nullptr, rc, "device allocation for %zu units failed", u);
    }
    *out = v;
    return ADDER_OK;
}

extern "C" void adder_stream_destroy(AdderStream *v) { stream_free(v); }

extern "C" int adder_stream_reset(AdderStream *v) {
    if (!v) return ADDER_E_BAD_PARAMS;
    SHIPCHK(v, hipSetDevice(v->p.device_id));
    SHIPCHK(v, hipDeviceSynchronize());
    SHIPCHK(v, hipMemset(v->a.state, 0, (size_t)v->a.units * 8u));
    SHIPCHK(v, hipMemset(v->info_t, 0, (size_t)v->a.units * 8u));
    SHIPCHK(v, hipMemcpy(v->d_fold, &kEmptyFold, sizeof kEmptyFold, hipMemcpyHostToDevice));
    v->fold = kEmptyFold;
    return ADDER_OK;
}

extern "C" const char *adder_stream_last_error(const AdderStream *v) {
    return v ? v->err.c_str() : g_stream_create_error.c_str();
}

// d_out == nullptr: the info fold; otherwise the migration
static int run(AdderStream *v, bool info, int source, const void *d_in, uint64_t n, void *d_out, uint64_t *bad_index,
               uint64_t *n_consumed, hipStream_t stream) {
    if (!v) return ADDER_E_BAD_PARAMS;
    if (bad_index) *bad_index = ADDER_STREAM_NO_BAD_EVENT;
    if (n_consumed) *n_consumed = 0;
    if (n > (uint64_t)INT32_MAX)
        return sfail(v, ADDER_E_BAD_PARAMS, "%llu events in one call (at most 2^31 - 1)", (unsigned long long)n);
    if (n > 0 && (!d_in || (!info && !d_out))) return sfail(v, ADDER_E_BAD_PARAMS, "null buffer");
    if (n == 0) return ADDER_OK;
    SHIPCHK(v, hipSetDevice(v->p.device_id));
    int rc = ensure_scratch(v, n, info);
    if (rc != ADDER_OK) return rc;
    if (info) {
        StreamArgs a = v->a;
        a.state = v->info_t;
        a.round = 0u;  // main.rs:97-99: the raw time
        SHIPCHK(v, stream_info(a, v->info_absolute ? 1 : 0, source, d_in, n, v->fold.min, v->d_fold, v->s, stream));
        SHIPCHK(v, hipMemcpyAsync(v->h_fold, v->d_fold, sizeof(StreamFold), hipMemcpyDeviceToHost, stream));
    } else {
        SHIPCHK(v, stream_migrate(v->a, v->op, source, d_in, d_out, n, v->s, stream));
    }
    SHIPCHK(v, hipMemcpyAsync(v->h_sc, v->s.sc, sizeof(StreamScalars), hipMemcpyDeviceToHost, stream));
    SHIPCHK(v, hipStreamSynchronize(stream));
    if (info) v->fold = *v->h_fold;
    const StreamScalars sc = *v->h_sc;
    if (n_consumed) *n_consumed = sc.eof;
    if (sc.bad < sc.eof) {
        if (bad_index) *bad_index = sc.bad;
        return sfail(v, ADDER_STREAM_E_BAD_EVENT, "event %llu of the batch is outside the plane or its time does not "
                     "fit (T + t above 2^32 - 1, or t below the unit's previous time)", (unsigned long long)sc.bad);
    }
    return ADDER_OK;
}

extern "C" int adder_stream_migrate_device(AdderStream *v, const AdderEvent *d_in, uint64_t n, AdderEvent *d_out,
                                           uint64_t *bad_index, void *stream) {
    return run(v, false, kSrcEvents, d_in, n, d_out, bad_index, nullptr, (hipStream_t)stream);
}

extern "C" int adder_stream_migrate_wire_device(AdderStream *v, const uint8_t *d_wire, uint64_t n_records,
                                                uint8_t *d_out, uint64_t *bad_index, uint64_t *n_consumed,
                                                void *stream) {
    if (!v) return ADDER_E_BAD_PARAMS;
    return run(v, false, wire_source(v->p.channels), d_wire, n_records, d_out, bad_index, n_consumed, (hipStream_t)stream);
}

extern "C" int adder_stream_info_device(AdderStream *v, const AdderEvent *d_events, uint64_t n, uint64_t *bad_index,
                                        void *stream) {
    return run(v, true, kSrcEvents, d_events, n, nullptr, bad_index, nullptr, (hipStream_t)stream);
}

extern "C" int adder_stream_info_wire_device(AdderStream *v, const uint8_t *d_wire, uint64_t n_records,
                                             uint64_t *bad_index, uint64_t *n_consumed, void *stream) {
    if (!v) return ADDER_E_BAD_PARAMS;
    return run(v, true, wire_source(v->p.channels), d_wire, n_records, nullptr, bad_index, n_consumed, (hipStream_t)stream);
}

static int run_host(AdderStream *v, bool info, int source, const void *in, uint64_t n, void *out, uint64_t *bad_index,
                    uint64_t *n_consumed) {
    if (!v) return ADDER_E_BAD_PARAMS;
    if (n > (uint64_t)INT32_MAX) return sfail(v, ADDER_E_BAD_PARAMS, "too many events in one call");
    if (n > 0 && (!in || (!info && !out))) return sfail(v, ADDER_E_BAD_PARAMS, "null buffer");
    SHIPCHK(v, hipSetDevice(v->p.device_id));
    const size_t rb = wire_record_bytes(source);
    if (!info) SHIPCHK(v, api_grow(&v->d_out, &v->d_out_cap, n * rb + 1u));
    SHIPCHK(v, api_stage_input(&v->d_in, &v->d_in_cap, in, n * rb, v->stream));
    uint64_t bad = ADDER_STREAM_NO_BAD_EVENT, consumed = n;
    const int rc = run(v, info, source, v->d_in, n, info ? nullptr : v->d_out, &bad, source == kSrcEvents ? nullptr : &consumed,
             v->stream);
    if (bad_index) *bad_index = bad;
    if (n_consumed) *n_consumed = n ? consumed : 0;
    if (!info && (rc == ADDER_OK || rc == ADDER_STREAM_E_BAD_EVENT)) {
        const uint64_t done = bad < consumed ? bad : consumed;
        if (done) SHIPCHK(v, hipMemcpy(out, v->d_out, done * rb, hipMemcpyDeviceToHost));
    }
    return rc;
}

extern "C" int adder_stream_migrate_host(AdderStream *v, const AdderEvent *in, uint64_t n, AdderEvent *out,
                                         uint64_t *bad_index) {
    return run_host(v, false, kSrcEvents, in, n, out, bad_index, nullptr);
}

extern "C" int adder_stream_migrate_wire_host(AdderStream *v, const uint8_t *wire, uint64_t n_records, uint8_t *out,
                                              uint64_t *bad_index, uint64_t *n_consumed) {
    if (!v) return ADDER_E_BAD_PARAMS;
    return run_host(v, false, wire_source(v->p.channels), wire, n_records, out, bad_index, n_consumed);
}

extern "C" int adder_stream_info_host(AdderStream *v, const AdderEvent *events, uint64_t n, uint64_t *bad_index) {
    return run_host(v, true, kSrcEvents, events, n, nullptr, bad_index, nullptr);
}

extern "C" int adder_stream_info_wire_host(AdderStream *v, const uint8_t *wire, uint64_t n_records, uint64_t *bad_index,
                                           uint64_t *n_consumed) {
    if (!v) return ADDER_E_BAD_PARAMS;
    return run_host(v, true, wire_source(v->p.channels), wire, n_records, nullptr, bad_index, n_consumed);
}

extern "C" int adder_stream_info_range(const AdderStream *v, double *min_intensity, double *max_intensity,
                                       uint64_t *n_events) {
    if (!v) return ADDER_E_BAD_PARAMS;
    if (min_intensity) *min_intensity = v->fold.min;
    if (max_intensity) memcpy(max_intensity, &v->fold.max_bits, 8);
    if (n_events) *n_events = v->fold.count;
    return ADDER_OK;
}

// Rust's {:.4}: the exact decimal expansion rounded half to even, as glibc's %.4f; the specials are spelled
// "inf", "-inf" and "NaN"
static std::string rust_f4(double x) {
    if (std::isnan(x)) return "NaN";
    if (std::isinf(x)) return x < 0 ? "-inf" : "inf";
    char buf[400];
    snprintf(buf, sizeof buf, "%.4f", x);
    return buf;
}

extern "C" size_t adder_stream_format_report(const AdderStreamParams *p, uint32_t header_bytes, uint64_t file_bytes,
                                             uint64_t n_events, int dynamic_range, double min_intensity,
                                             double max_intensity, char *out, size_t cap) {
    if (!p) return 0;
    static const char *const cams[] = {"FramedU8", "FramedU16", "FramedU32", "FramedU64", "FramedF32",
                                       "FramedF64", "Dvs",       "DavisU8",   "Atis",      "Asint"};
    static const char *const modes[] = {"DeltaT", "AbsoluteT", "Mixed"};
    const uint64_t volume = (uint64_t)p->width * p->height * p->channels;
    std::string r = "Dimensions\n";
    r += "\tWidth: " + std::to_string(p->width) + "\n";
    r += "\tHeight: " + std::to_string(p->height) + "\n";
    r += "\tColor channels: " + std::to_string(p->channels) + "\n";
    r += "Source camera: " + (p->source_camera < 10u ? std::string(cams[p->source_camera])
                                                     : "Unknown(" + std::to_string(p->source_camera) + ")") + "\n";
    r += "AD\xce\x94" "ER transcoder parameters\n";
    r += "\tCodec version: " + std::to_string(p->codec_version) + "\n";
    // a v0 / v1 header has no time-mode field and the reference's decoder keeps TimeMode::default() = AbsoluteT
    // there (decoder.rs:119-123), which is what its report prints
    r += "\tTime mode: " + std::string(p->codec_version < 2 ? modes[1] : modes[p->time_mode < 3 ? p->time_mode : 0]) + "\n";
    r += "\tTicks per second: " + std::to_string(p->tps) + "\n";
    r += "\tReference ticks per source interval: " + std::to_string(p->ref_interval) + "\n";
    r += "\t\xce\x94t_max: " + std::to_string(p->delta_t_max) + "\n";
    r += "File metadata\n";
    r += "\tFile size: " + std::to_string(file_bytes) + "\n";
    r += "\tHeader size: " + std::to_string(header_bytes) + "\n";
    r += "\tAD\xce\x94" "ER event count: " + std::to_string(n_events) + "\n";
    r += "\tEvents per pixel channel: " + std::to_string(volume ? n_events / volume : 0) + "\n";
    if (dynamic_range) {
        // D_SHIFT[128] is 0 (adder-codec-core lib.rs:220-231), so the theoretical ratio is 0 and its logarithms -inf
        const double theory = 0.0 / (1.0 / (double)p->delta_t_max);
        const double real = max_intensity / min_intensity;
        r += "Dynamic range\n";
        r += "\tTheoretical range:\n";
        r += "\t\t" + rust_f4(10.0 * log10(theory)) + " dB (power)\n";
        r += "\t\t" + rust_f4(log2(theory)) + " bits\n";
        r += "\tRealized range:\n";
        r += "\t\t" + rust_f4(10.0 * log10(real)) + " dB (power)\n";
        r += "\t\t" + rust_f4(log2(real)) + " bits\n";
    }
    if (out && r.size() <= cap) memcpy(out, r.data(), r.size());
    return r.size();
}
