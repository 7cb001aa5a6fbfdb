// adder_prophesee_api.cpp -- C-ABI of the Prophesee .dat -> ADDER transcoder (include/adder_prophesee.h): the .dat
// header parser and record decoder, the group scan of Prophesee::consume, the per-pixel camera state and push
// scratch in HBM, the launches of adder_prophesee.hip and the inner sparse context.  No CPU fallback.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <new>
#include <utility>
#include <vector>

#include "../../include/adder_prophesee.h"
#include "adder_exp.hpp"
#include "adder_log1p.hpp"
#include "adder_prophesee_kernels.h"
#include "adder_source_util.hpp"

using namespace adder;

static thread_local std::string g_pph_create_error;

namespace {

enum Phase { kCreated = 0, kStarted = 1, kFinished = 2 };
constexpr uint32_t kPphMaxDepth = 31;  // kMaxDepthLimit (adder_pixel.hpp)

// Rust's str::parse::<u32>: an optional '+', then decimal digits only, no overflow
bool parse_u32(const uint8_t *s, size_t n, uint32_t *out) {
    size_t i = 0;
    if (n > 0 && s[0] == '+') i = 1;
    if (i == n) return false;
    uint64_t v = 0;
    for (; i < n; ++i) {
        if (s[i] < '0' || s[i] > '9') return false;
        v = v * 10u + (uint64_t)(s[i] - '0');
        if (v > 0xffffffffull) return false;
    }
    *out = (uint32_t)v;
    return true;
}

}  // namespace

struct AdderProphesee {
    AdderPropheseeParams p{};
    AdderHipCtx *ctx = nullptr;
    PphArgs a{};
    hipStream_t stream = nullptr;  // the host-pointer forms' stream
    int phase = kCreated;
    uint32_t running_t = 0, group_start_t = 0;
    uint64_t base = 0;     // stream index of pend[0]
    uint64_t pushed = 0;   // records pushed so far
    uint64_t eps = 0;      // events per step at most (max_depth + 3)
    // the open group's records (device), and a second buffer of the same size to move the tail into
    uint8_t *pend = nullptr, *pend2 = nullptr;
    uint64_t pend_n = 0, pend_cap = 0;
    PphScratch s{};    // push scratch
    StepBuffer steps;  // 2 * s.chain.cap (and at least units, for end_events)
    PphScalars *h_sc = nullptr;        // pinned
    uint32_t *h_t = nullptr;           // pinned: the pushed records' t
    uint64_t h_t_cap = 0;
    // host-pointer forms
    void *d_in = nullptr, *d_out = nullptr;
    size_t d_in_cap = 0, d_out_cap = 0;
    std::string err;
};

static int pfail(AdderProphesee *v, int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    api_fail(v ? v->err : g_pph_create_error, code, fmt, ap);
    va_end(ap);
    return code;
}

#define PHIPCHK(v, expr) ADDER_HIPCHK(pfail, v, expr, #expr)

// ------------------------------------------------------------------------------------------ header, records, groups
extern "C" int adder_prophesee_parse_header(const uint8_t *b, size_t len, uint64_t file_size, AdderPropheseeHeader *out) {
    if ((!b && len) || !out) return ADDER_E_BAD_PARAMS;
    uint32_t size[2] = {70u, 100u};  // height, width: unwrap_or(70), unwrap_or(100)
    size_t pos = 0, lines = 0;
    for (;;) {  // :375-397
        if (pos >= len || b[pos] != '%') break;
        size_t end = pos;
        while (end < len && b[end] != '\n') ++end;
        if (end == len && len < file_size) return ADDER_E_OUT_CAPACITY;  // the line may go on past the buffer
        const size_t line_end = end < len ? end + 1 : end;               // the '\n' belongs to the line
        // split on ' ' and '\t'
        std::vector<std::pair<size_t, size_t>> words;
        size_t w0 = pos;
        for (size_t i = pos; i < line_end; ++i)
            if (b[i] == ' ' || b[i] == '\t') {
                words.emplace_back(w0, i);
                w0 = i + 1;
            }
        words.emplace_back(w0, line_end);
        if (words.size() > 1) {
            const size_t n1 = words[1].second - words[1].first;
            const uint8_t *w1 = b + words[1].first;
            const int which = (n1 == 6 && !memcmp(w1, "Height", 6)) ? 0 : (n1 == 5 && !memcmp(w1, "Width", 5)) ? 1 : -1;
            if (which >= 0) {  // line_to_hw (:424-435): words.get(2).unwrap(), word.last().unwrap() panic
                if (words.size() < 3 || words[2].second == words[2].first) return ADDER_E_BAD_PARAMS;
                size_t s = words[2].first, e = words[2].second;
                if (b[e - 1] == '\n') --e;
                uint32_t v = 0;
                size[which] = parse_u32(b + s, e - s, &v) ? v : (which == 0 ? 70u : 100u);
            }
        }
        ++lines;
        pos = line_end;
    }
    AdderPropheseeHeader h{};
    if (lines > 0) {  // :401-414: two bytes, ev_size 8 and ev_type 0 or 12, else the reference panics
        if (pos + 2 > len) return len < file_size ? ADDER_E_OUT_CAPACITY : ADDER_E_BAD_PARAMS;
        h.ev_type = b[pos];
        h.ev_size = b[pos + 1];
        if (h.ev_size != 8 || (h.ev_type != 0 && h.ev_type != 12)) return ADDER_E_BAD_PARAMS;
        pos += 2;
    }
    // PlaneSize::new(width as u16, height as u16, 1) refuses a zero dimension
    h.width = (uint16_t)size[1];
    h.height = (uint16_t)size[0];
    if (h.width == 0 || h.height == 0) return ADDER_E_BAD_PARAMS;
    if (pos > 0xffffffffull) return ADDER_E_BAD_PARAMS;
    h.header_bytes = (uint32_t)pos;
    h.header_lines = (uint8_t)std::min<size_t>(lines, 255);
    *out = h;
    return ADDER_OK;
}

extern "C" void adder_prophesee_decode(const uint8_t *rec, uint64_t n, AdderPropheseeEvent *out) {
    for (uint64_t i = 0; i < n; ++i) {
        uint32_t t, d;
        memcpy(&t, rec + 8 * i, 4);
        memcpy(&d, rec + 8 * i + 4, 4);
        AdderPropheseeEvent e{};
        e.t = t;
        e.x = (uint16_t)(d & 0x3ffu);
        e.y = (uint16_t)((d & 0xfffc000u) >> 14);
        e.p = (uint8_t)((d & 0x10000000u) >> 28);
        out[i] = e;
    }
}

// consume()'s reading loop (:142-170) over t values with a stride; returns the records that complete groups.  Blocks
// of 256 records whose largest t does not pass the limit (and the limit has not wrapped) close nothing and only raise
// running_t: they take one vectorisable max; a block that may close a group is read record by record.
template <size_t STRIDE>
static uint64_t scan_groups(const uint8_t *t_bytes, uint64_t n, uint32_t *group_start_t, uint32_t *running_t,
                            uint64_t *groups) {
    constexpr uint64_t B = 256;
    auto load = [&](uint64_t i) {
        uint32_t t;
        memcpy(&t, t_bytes + i * STRIDE, 4);
        return t;
    };
    uint32_t start = *group_start_t, rt = *running_t;
    uint32_t limit = start + ADDER_PROPHESEE_VIEW_INTERVAL;  // u32 wrapping
    uint64_t done = 0, g = 0;
    for (uint64_t i = 0; i < n;) {
        if (i + B <= n && limit >= start) {
            uint32_t m = 0;
            for (uint64_t k = 0; k < B; ++k) m = std::max(m, load(i + k));
            if (m <= limit) {
                rt = std::max(rt, m);
                i += B;
                continue;
            }
        }
        for (const uint64_t e = std::min(n, i + B); i < e; ++i) {
            const uint32_t t = load(i);
            if (t > rt) rt = t;
            if (t > limit) {  // the record closes its group; the next group starts at running_t
                done = i + 1;
                ++g;
                start = rt;
                limit = start + ADDER_PROPHESEE_VIEW_INTERVAL;
            }
        }
    }
    *group_start_t = start;
    *running_t = rt;
    if (groups) *groups = g;
    return done;
}

extern "C" uint64_t adder_prophesee_scan_groups(const uint8_t *records, uint64_t n, uint32_t *group_start_t,
                                                uint32_t *running_t, uint64_t *groups) {
    if (!group_start_t || !running_t || (!records && n)) return 0;
    return scan_groups<8>(records, n, group_start_t, running_t, groups);
}

// ------------------------------------------------------------------------------------------ lifecycle
static void pph_free(AdderProphesee *v) {
    if (!v) return;
    (void)hipSetDevice(v->p.device_id);
    if (v->stream) (void)hipStreamSynchronize(v->stream);
    (void)hipDeviceSynchronize();
    chain_free(v->s.chain);
    api_free_all({v->a.cur_t, v->a.nxt_t, v->a.cur_ln, v->a.nxt_ln, v->s.sc, v->pend, v->pend2, v->steps.p, v->d_in,
                  v->d_out});
    if (v->h_sc) (void)hipHostFree(v->h_sc);
    if (v->h_t) (void)hipHostFree(v->h_t);
    if (v->ctx) adder_hip_destroy(v->ctx);
    if (v->stream) (void)hipStreamDestroy(v->stream);
    delete v;
}

// Prophesee::new (:56-113) + .crf(c): a Continuous context with the source's time parameters; the camera state
// back to last t = 2, last ln = ln_1p(128 / 255)
static int open_ctx(AdderProphesee *v) {
    const AdderPropheseeParams &p = v->p;
    AdderHipParams hp;
    adder_hip_default_params(&hp, p.width, p.height, 1);
    hp.pixel_mode = ADDER_MODE_CONTINUOUS;
    hp.ref_time = p.ref_time;
    hp.delta_t_max = p.ref_time * 2u;
    hp.chunk_rows = 1;
    // the reference's arena grows without bound; a camera pixel at crf 0 (c_thresh 0) stores more than the framed
    // default of 16 nodes, so the context takes the largest depth the kernels support
    hp.max_depth = kPphMaxDepth;
    hp.device_id = p.device_id;
    // Crf::new(None) is quality 3: its limits hold, but without a .crf(c) call no pixel is reset to its baseline
    const int rc = source_open_ctx(&v->ctx, hp, p.crf == ADDER_PROPHESEE_NO_CRF ? 3 : p.crf,
                                   p.crf == ADDER_PROPHESEE_NO_CRF ? -1 : p.crf, v->a.units, &v->eps, v->err);
    if (rc != ADDER_OK) return rc;
    PHIPCHK(v, pph_init_state(v->a, v->stream));
    PHIPCHK(v, hipStreamSynchronize(v->stream));
    v->phase = kCreated;
    v->running_t = v->group_start_t = 0;
    v->base = v->pushed = v->pend_n = 0;
    return ADDER_OK;
}

extern "C" int adder_prophesee_create(const AdderPropheseeParams *p, AdderProphesee **out) {
    if (!p || !out) return pfail(nullptr, ADDER_E_BAD_PARAMS, "null argument");
    *out = nullptr;
    if (p->abi_version != ADDER_PROPHESEE_ABI_VERSION)
        return pfail(nullptr, ADDER_E_BAD_PARAMS, "abi_version %u, this library is %u", p->abi_version,
                     ADDER_PROPHESEE_ABI_VERSION);
    if (p->width == 0 || p->height == 0) return pfail(nullptr, ADDER_E_BAD_PARAMS, "plane %ux%u", p->width, p->height);
    if (p->ref_time == 0 || p->ref_time > 0x7fffffffu)
        return pfail(nullptr, ADDER_E_BAD_PARAMS, "ref_time %u (1 .. 2^31 - 1)", p->ref_time);
    if (p->crf != ADDER_PROPHESEE_NO_CRF && (p->crf < 0 || p->crf > 9))
        return pfail(nullptr, ADDER_E_BAD_PARAMS, "crf %d (0..9, or ADDER_PROPHESEE_NO_CRF)", p->crf);
    if (const int rc = api_check_device(p->device_id, g_pph_create_error)) return rc;
    AdderProphesee *v = new (std::nothrow) AdderProphesee();
    if (!v) return pfail(nullptr, ADDER_E_BAD_PARAMS, "out of host memory");
    v->p = *p;
    PphArgs &a = v->a;
    a.width = p->width;
    a.height = p->height;
    a.units = (uint32_t)p->width * p->height;
    a.key_bits = key_bits_for(a.units);
    a.ref_time = p->ref_time;
    a.theta = 0.02;  // camera_theta (:108)
    a.ln_mid = dvs_log1p(128.0 / 255.0);
    const size_t u = a.units;
    int rc = ADDER_OK;
    auto mk = [&](void **b, size_t bytes) {
        if (rc == ADDER_OK && hipMalloc(b, bytes) != hipSuccess) rc = ADDER_E_HIP;
    };
    if (hipSetDevice(p->device_id) != hipSuccess) rc = ADDER_E_HIP;
    mk((void **)&a.cur_t, u * 4u);
    mk((void **)&a.nxt_t, u * 4u);
    mk((void **)&a.cur_ln, u * 8u);
    mk((void **)&a.nxt_ln, u * 8u);
    mk((void **)&v->s.sc, sizeof(PphScalars));
    if (rc == ADDER_OK && hipHostMalloc((void **)&v->h_sc, sizeof(PphScalars), hipHostMallocDefault) != hipSuccess)
        rc = ADDER_E_HIP;
    if (rc == ADDER_OK && hipStreamCreateWithFlags(&v->stream, hipStreamNonBlocking) != hipSuccess) rc = ADDER_E_HIP;
    if (rc != ADDER_OK) {
        pph_free(v);
        return pfail(nullptr, rc, "device allocation for %zu pixels failed", u);
    }
    if ((rc = open_ctx(v)) != ADDER_OK) {
        g_pph_create_error = v->err;
        pph_free(v);
        return rc;
    }
    *out = v;
    return ADDER_OK;
}

extern "C" void adder_prophesee_destroy(AdderProphesee *v) { pph_free(v); }

extern "C" int adder_prophesee_reset(AdderProphesee *v) {
    if (!v) return ADDER_E_BAD_PARAMS;
    PHIPCHK(v, hipSetDevice(v->p.device_id));
    PHIPCHK(v, hipDeviceSynchronize());
    return open_ctx(v);
}

extern "C" const char *adder_prophesee_last_error(const AdderProphesee *v) {
    return v ? v->err.c_str() : g_pph_create_error.c_str();
}

extern "C" uint64_t adder_prophesee_events_per_step(const AdderProphesee *v) { return v ? v->eps : 0; }

extern "C" int adder_prophesee_state(const AdderProphesee *v, uint32_t *running_t, uint32_t *group_start_t,
                                     uint64_t *open_records, uint64_t *records_pushed) {
    if (!v) return ADDER_E_BAD_PARAMS;
    if (running_t) *running_t = v->running_t;
    if (group_start_t) *group_start_t = v->group_start_t;
    if (open_records) *open_records = v->pend_n;
    if (records_pushed) *records_pushed = v->pushed;
    return ADDER_OK;
}

extern "C" int adder_prophesee_pixel_state(AdderProphesee *v, uint32_t *last_t, double *last_ln) {
    if (!v) return ADDER_E_BAD_PARAMS;
    PHIPCHK(v, hipSetDevice(v->p.device_id));
    // (every push and finish has waited for its stream before it returned)
    if (last_t) PHIPCHK(v, hipMemcpy(last_t, v->a.cur_t, (size_t)v->a.units * 4u, hipMemcpyDeviceToHost));
    if (last_ln) PHIPCHK(v, hipMemcpy(last_ln, v->a.cur_ln, (size_t)v->a.units * 8u, hipMemcpyDeviceToHost));
    return ADDER_OK;
}

extern "C" int adder_prophesee_running_intensities(AdderProphesee *v, uint8_t *dst) {
    if (!v || !dst) return ADDER_E_BAD_PARAMS;
    const int rc = adder_hip_running_intensities(v->ctx, dst);
    return rc == ADDER_OK ? rc : pfail(v, rc, "%s", adder_hip_last_error(v->ctx));
}

// ------------------------------------------------------------------------------------------ start, push, finish
extern "C" int adder_prophesee_start(AdderProphesee *v, AdderEvent *out, uint64_t out_cap, uint64_t *n_out) {
    if (!v) return ADDER_E_BAD_PARAMS;
    if (n_out) *n_out = 0;
    if (v->phase != kCreated) return pfail(v, ADDER_PROPHESEE_E_ORDER, "start: already started (reset first)");
    const uint64_t per = adder_hip_max_events_per_frame(v->ctx);
    if (!out || out_cap < 2 * per) {
        if (n_out) *n_out = 2 * per;
        return pfail(v, ADDER_E_OUT_CAPACITY, "start: %llu events of room needed", (unsigned long long)(2 * per));
    }
    // :117-131: integrate_matrix twice over the start intensities (128); the second must fire every pixel once
    std::vector<uint8_t> frame((size_t)v->a.units, 128);
    size_t n1 = 0, n2 = 0;
    int rc = adder_hip_integrate(v->ctx, frame.data(), v->a.width, (float)v->p.ref_time, out, out_cap, &n1, nullptr);
    if (rc == ADDER_OK)
        rc = adder_hip_integrate(v->ctx, frame.data(), v->a.width, (float)v->p.ref_time, out + n1, out_cap - n1, &n2,
                                 nullptr);
    if (rc != ADDER_OK) return pfail(v, rc, "start frames: %s", adder_hip_last_error(v->ctx));
    if (n_out) *n_out = n1 + n2;
    v->phase = kFinished;  // nothing but reset after a failed start
    if (n2 != v->a.units)
        return pfail(v, ADDER_E_BAD_PARAMS, "the second start frame made %zu events, not one per pixel (%u)", n2,
                     v->a.units);
    v->phase = kStarted;
    v->running_t = v->group_start_t = 2;
    return ADDER_OK;
}

static int ensure_scratch(AdderProphesee *v, uint64_t n) {
    PHIPCHK(v, chain_reserve(v->s.chain, n, 0u));
    PHIPCHK(v, steps_reserve(v->steps, 2u * v->s.chain.cap));
    return ADDER_OK;
}

// the open group's buffers hold `need` records; the carried ones are kept
static int ensure_pend(AdderProphesee *v, uint64_t need, hipStream_t s) {
    if (need <= v->pend_cap) return ADDER_OK;
    const uint64_t c = need + need / 2u;
    uint8_t *a = nullptr, *b = nullptr;
    PHIPCHK(v, hipMalloc((void **)&a, c * 8u));
    PHIPCHK(v, hipMalloc((void **)&b, c * 8u));
    if (v->pend_n) PHIPCHK(v, hipMemcpyAsync(a, v->pend, v->pend_n * 8u, hipMemcpyDeviceToDevice, s));
    PHIPCHK(v, hipStreamSynchronize(s));
    if (v->pend) PHIPCHK(v, hipFree(v->pend));
    if (v->pend2) PHIPCHK(v, hipFree(v->pend2));
    v->pend = a;
    v->pend2 = b;
    v->pend_cap = c;
    return ADDER_OK;
}

static int push(AdderProphesee *v, const uint8_t *d_rec, const uint8_t *h_rec, uint64_t n, AdderEvent *d_out,
                uint64_t out_cap, uint64_t *n_out, uint64_t *bad_index, hipStream_t s) {
    if (n_out) *n_out = 0;
    if (bad_index) *bad_index = ADDER_PROPHESEE_NO_BAD_RECORD;
    if (v->phase != kStarted)
        return pfail(v, ADDER_PROPHESEE_E_ORDER, v->phase == kCreated ? "push before start" : "push after finish");
    if (n > (uint64_t)INT32_MAX) return pfail(v, ADDER_E_BAD_PARAMS, "%llu records in one push (at most 2^31 - 1)",
                                              (unsigned long long)n);
    if (out_cap > 0 && !d_out) return pfail(v, ADDER_E_BAD_PARAMS, "null output with capacity");
    if (n == 0) return ADDER_OK;
    if (!d_rec) return pfail(v, ADDER_E_BAD_PARAMS, "null records");
    PHIPCHK(v, hipSetDevice(v->p.device_id));
    // the group scan runs on the host over the records' t
    uint32_t start = v->group_start_t, rt = v->running_t;
    uint64_t done;
    if (h_rec) {
        done = scan_groups<8>(h_rec, n, &start, &rt, nullptr);
    } else {
        if (n > v->h_t_cap) {
            if (v->h_t) PHIPCHK(v, hipHostFree(v->h_t));
            v->h_t = nullptr;
            v->h_t_cap = 0;
            PHIPCHK(v, hipHostMalloc((void **)&v->h_t, n * 4u, hipHostMallocDefault));
            v->h_t_cap = n;
        }
        int rc_ = ensure_scratch(v, n);  // keys0 holds the records' t for the copy
        if (rc_ != ADDER_OK) return rc_;
        PHIPCHK(v, pph_times(d_rec, n, v->s.chain.keys0, s));
        PHIPCHK(v, hipMemcpyAsync(v->h_t, v->s.chain.keys0, n * 4u, hipMemcpyDeviceToHost, s));
        PHIPCHK(v, hipStreamSynchronize(s));
        done = scan_groups<4>((const uint8_t *)v->h_t, n, &start, &rt, nullptr);
    }
    int rc = ensure_pend(v, v->pend_n + n, s);
    if (rc != ADDER_OK) return rc;
    PHIPCHK(v, hipMemcpyAsync(v->pend + v->pend_n * 8u, d_rec, n * 8u, hipMemcpyDeviceToDevice, s));
    const uint64_t m = done ? v->pend_n + done : 0;  // records of the groups this push completes
    uint64_t total = 0;
    if (m) {
        if (m > (uint64_t)INT32_MAX) return pfail(v, ADDER_E_BAD_PARAMS, "an open group of more than 2^31 - 1 records");
        if ((rc = ensure_scratch(v, m)) != ADDER_OK) return rc;
        PHIPCHK(v, pph_generate(v->a, v->pend, m, v->s, s));
        PHIPCHK(v, hipMemcpyAsync(v->h_sc, v->s.sc, sizeof(PphScalars), hipMemcpyDeviceToHost, s));
        PHIPCHK(v, hipStreamSynchronize(s));
        const PphScalars sc = *v->h_sc;
        if (sc.bad != ~0ull) {
            if (bad_index) *bad_index = v->base + sc.bad;
            return pfail(v, ADDER_PROPHESEE_E_BAD_RECORD, "record %llu of the stream is outside the %ux%u plane",
                         (unsigned long long)(v->base + sc.bad), v->a.width, v->a.height);
        }
        const uint64_t need = sc.steps * v->eps;
        if (out_cap < need) {
            if (n_out) *n_out = need;
            return pfail(v, ADDER_E_OUT_CAPACITY, "%llu steps may make %llu events; the buffer holds %llu",
                         (unsigned long long)sc.steps, (unsigned long long)need, (unsigned long long)out_cap);
        }
        PHIPCHK(v, pph_emit(v->a, m, v->s, v->steps.p, s));
        if (sc.steps) {
            size_t got = 0;
            rc = adder_hip_integrate_sparse_device(v->ctx, v->steps.p, sc.steps, d_out, out_cap, &got, s);
            if (rc != ADDER_OK) {
                v->phase = kFinished;  // the pixels have been stepped: only reset helps
                return pfail(v, rc, "integrate_sparse: %s", adder_hip_last_error(v->ctx));
            }
            total = got;
        }
        const uint64_t rest = v->pend_n + n - m;
        if (rest) {
            PHIPCHK(v, hipMemcpyAsync(v->pend2, v->pend + m * 8u, rest * 8u, hipMemcpyDeviceToDevice, s));
            std::swap(v->pend, v->pend2);
        }
        PHIPCHK(v, hipStreamSynchronize(s));
        v->pend_n = rest;
        v->base += m;
    } else {
        PHIPCHK(v, hipStreamSynchronize(s));
        v->pend_n += n;
    }
    v->group_start_t = start;
    v->running_t = rt;
    v->pushed += n;
    if (n_out) *n_out = total;
    return ADDER_OK;
}

extern "C" int adder_prophesee_push_device(AdderProphesee *v, const uint8_t *d_records, uint64_t n, AdderEvent *d_out,
                                           uint64_t out_cap, uint64_t *n_out, uint64_t *bad_index, void *stream) {
    if (!v) return ADDER_E_BAD_PARAMS;
    return push(v, d_records, nullptr, n, d_out, out_cap, n_out, bad_index, (hipStream_t)stream);
}

extern "C" int adder_prophesee_push_host(AdderProphesee *v, const uint8_t *records, uint64_t n, AdderEvent *out,
                                         uint64_t out_cap, uint64_t *n_out, uint64_t *bad_index) {
    if (!v) return ADDER_E_BAD_PARAMS;
    if (n_out) *n_out = 0;
    if (n > 0 && !records) return pfail(v, ADDER_E_BAD_PARAMS, "null records");
    if (out_cap > 0 && !out) return pfail(v, ADDER_E_BAD_PARAMS, "null output");
    if (n > (uint64_t)INT32_MAX) return pfail(v, ADDER_E_BAD_PARAMS, "too many records in one push");
    PHIPCHK(v, hipSetDevice(v->p.device_id));
    // at most 2 steps per record in this push and the open group
    const uint64_t most = 2u * (v->pend_n + n) * v->eps;
    const uint64_t dcap = out_cap < most ? out_cap : most;
    PHIPCHK(v, api_grow(&v->d_in, &v->d_in_cap, n * 8u + 8u));
    PHIPCHK(v, api_grow(&v->d_out, &v->d_out_cap, dcap * sizeof(AdderEvent) + 16u));
    if (n) PHIPCHK(v, hipMemcpyAsync(v->d_in, records, n * 8u, hipMemcpyHostToDevice, v->stream));
    uint64_t got = 0;
    const int rc = push(v, n ? (const uint8_t *)v->d_in : nullptr, records, n, (AdderEvent *)v->d_out, dcap, &got, bad_index,
              v->stream);
    if (n_out) *n_out = got;
    if (rc == ADDER_OK && got) PHIPCHK(v, hipMemcpy(out, v->d_out, got * sizeof(AdderEvent), hipMemcpyDeviceToHost));
    return rc;
}

extern "C" int adder_prophesee_finish_device(AdderProphesee *v, AdderEvent *d_out, uint64_t out_cap, uint64_t *n_out,
                                             void *stream) {
    if (!v) return ADDER_E_BAD_PARAMS;
    if (n_out) *n_out = 0;
    if (v->phase != kStarted)
        return pfail(v, ADDER_PROPHESEE_E_ORDER, v->phase == kCreated ? "finish before start" : "finish twice");
    const uint64_t need = (uint64_t)v->a.units * v->eps;
    if (!d_out || out_cap < need) {
        if (n_out) *n_out = need;
        return pfail(v, ADDER_E_OUT_CAPACITY, "end_events may make %llu events", (unsigned long long)need);
    }
    PHIPCHK(v, hipSetDevice(v->p.device_id));
    const hipStream_t s = (hipStream_t)stream;
    PHIPCHK(v, steps_reserve(v->steps, v->a.units));
    PHIPCHK(v, pph_end_steps(v->a, v->running_t, v->steps.p, v->s.sc, s));
    PHIPCHK(v, hipMemcpyAsync(v->h_sc, v->s.sc, sizeof(PphScalars), hipMemcpyDeviceToHost, s));
    PHIPCHK(v, hipStreamSynchronize(s));
    if (v->h_sc->end_bad) {
        v->phase = kFinished;  // the reference stops at its assert: nothing but reset after it
        return pfail(v, ADDER_PROPHESEE_E_END_ASSERT, "end_events: %llu pixels have last t == running_t (%u); the "
                     "reference asserts running_t - last_t > 0", (unsigned long long)v->h_sc->end_bad, v->running_t);
    }
    size_t got = 0;
    const int rc = adder_hip_integrate_sparse_device(v->ctx, v->steps.p, v->a.units, d_out, out_cap, &got, s);
    v->phase = kFinished;
    if (rc != ADDER_OK) return pfail(v, rc, "integrate_sparse: %s", adder_hip_last_error(v->ctx));
    v->pend_n = 0;  // the open group is dropped
    if (n_out) *n_out = got;
    return ADDER_OK;
}

extern "C" int adder_prophesee_finish_host(AdderProphesee *v, AdderEvent *out, uint64_t out_cap, uint64_t *n_out) {
    if (!v) return ADDER_E_BAD_PARAMS;
    if (n_out) *n_out = 0;
    const uint64_t need = (uint64_t)v->a.units * v->eps;
    if (!out || out_cap < need) {
        if (n_out) *n_out = need;
        return pfail(v, ADDER_E_OUT_CAPACITY, "end_events may make %llu events", (unsigned long long)need);
    }
    PHIPCHK(v, hipSetDevice(v->p.device_id));
    PHIPCHK(v, api_grow(&v->d_out, &v->d_out_cap, need * sizeof(AdderEvent)));
    uint64_t got = 0;
    const int rc = adder_prophesee_finish_device(v, (AdderEvent *)v->d_out, need, &got, v->stream);
    if (rc != ADDER_OK) return rc;
    if (got) PHIPCHK(v, hipMemcpy(out, v->d_out, got * sizeof(AdderEvent), hipMemcpyDeviceToHost));
    if (n_out) *n_out = got;
    return ADDER_OK;
}

// ------------------------------------------------------------------------------------------ exp self-tests
extern "C" double adder_prophesee_exp(double x) { return adder_exp(x); }

extern "C" void adder_prophesee_exp_host(const double *x, double *y, uint64_t n) {
    for (uint64_t i = 0; i < n; ++i) y[i] = adder_exp(x[i]);
}

extern "C" int adder_prophesee_exp_device(const double *d_x, double *d_y, uint64_t n, int device_id) {
    if (hipSetDevice(device_id) != hipSuccess) return ADDER_E_NO_DEVICE;
    if (pph_exp_run(d_x, d_y, n, nullptr) != hipSuccess) return ADDER_E_HIP;
    return hipDeviceSynchronize() == hipSuccess ? ADDER_OK : ADDER_E_HIP;
}
