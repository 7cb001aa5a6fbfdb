// adder_dvs_api.cpp -- C-ABI of the ADDER -> DVS conversion (include/adder_dvs.h): header parsing, the per-unit
// state and call scratch in HBM, the launches of adder_dvs.hip, and the host helpers of the .dat / text writer
// (adder-to-dvs/src/main.rs:151-163, 486-554).  No CPU fallback.
#include <hip/hip_runtime.h>

#include <climits>
#include <new>

#include "../../include/adder_dvs.h"
#include "adder_api_util.hpp"
#include "adder_dvs_kernels.h"
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
    if (n == 0) return ADDER_OK;
    DHIPCHK(v, hipSetDevice(v->p.device_id));
    int rc = ensure_scratch(v, n);
    if (rc != ADDER_OK) return rc;
    DHIPCHK(v, dvs_convert(v->a, source, d_in, n, fmt, d_out, out_cap, v->s, stream));
    DHIPCHK(v, hipMemcpyAsync(v->h_sc, v->s.sc, sizeof(DvsScalars), hipMemcpyDeviceToHost, stream));
    DHIPCHK(v, hipStreamSynchronize(stream));
    const DvsScalars sc = *v->h_sc;
    if (n_out) *n_out = sc.total;
    if (n_consumed) *n_consumed = sc.eof;
    const bool bad = sc.bad < sc.eof;
    if (bad && bad_index) *bad_index = sc.bad;
    if (sc.total > out_cap)
        return dfail(v, ADDER_E_OUT_CAPACITY, "%llu DVS events do not fit in %llu", (unsigned long long)sc.total,
                     (unsigned long long)out_cap);
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
