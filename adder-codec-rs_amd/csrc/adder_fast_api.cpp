// adder_fast_api.cpp -- C-ABI of the dense FAST detector and the feature scores (include/adder_fast.h): argument
// checks, the call scratch in HBM (grown with api_grow, kept between calls), the launches of adder_fast.hip, and the
// host-side end of cv.rs:258-278 (the four counts and three ratios from a frame's integer sums).  No CPU fallback.
#include <hip/hip_runtime.h>

#include <new>

#include "../../include/adder_fast.h"
#include "adder_api_util.hpp"
#include "adder_fast_kernels.h"
#include "adder_fast_logic.hpp"

using namespace adder;

static thread_local std::string g_fast_create_error;

struct AdderFast {
    AdderFastParams p{};
    FastShape s{};
    hipStream_t stream = nullptr;  // the host-pointer forms' stream
    // call scratch
    uint8_t *mask = nullptr;
    size_t mask_cap = 0;
    uint8_t *score = nullptr;
    size_t score_cap = 0;
    uint32_t *offs = nullptr;
    size_t offs_cap = 0;
    void *temp = nullptr;
    size_t temp_cap = 0;
    FastFrameSums *d_sums = nullptr;
    size_t d_sums_cap = 0;
    FastFrameSums *h_sums = nullptr;  // pinned
    uint32_t h_sums_frames = 0;
    uint32_t *d_bad = nullptr;
    uint32_t *h_bad = nullptr;        // pinned
    // host-pointer forms: inputs and outputs
    void *d_in = nullptr;
    size_t d_in_cap = 0;
    void *d_pred = nullptr;
    size_t d_pred_cap = 0;
    uint8_t *d_omask = nullptr;
    size_t d_omask_cap = 0;
    uint8_t *d_oscore = nullptr;
    size_t d_oscore_cap = 0;
    uint32_t *d_oxy = nullptr;
    size_t d_oxy_cap = 0;
    std::string err;
};

static int ffail(AdderFast *f, int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    api_fail(f ? f->err : g_fast_create_error, code, fmt, ap);
    va_end(ap);
    return code;
}

#define FHIPCHK(f, expr) ADDER_HIPCHK(ffail, f, expr, #expr)

static void fast_free(AdderFast *f) {
    if (!f) return;
    (void)hipSetDevice(f->p.device_id);
    if (f->stream) (void)hipStreamSynchronize(f->stream);
    api_free_all({f->mask, f->score, f->offs, f->temp, f->d_sums, f->d_bad, f->d_in, f->d_pred, f->d_omask, f->d_oscore,
                  f->d_oxy});
    if (f->h_sums) (void)hipHostFree(f->h_sums);
    if (f->h_bad) (void)hipHostFree(f->h_bad);
    if (f->stream) (void)hipStreamDestroy(f->stream);
    delete f;
}

extern "C" int adder_fast_create(const AdderFastParams *p, AdderFast **out) {
    if (!p || !out) return ffail(nullptr, ADDER_E_BAD_PARAMS, "null argument");
    *out = nullptr;
    if (p->abi_version != ADDER_FAST_ABI_VERSION)
        return ffail(nullptr, ADDER_E_BAD_PARAMS, "abi_version %u, this library is %u", p->abi_version,
                     ADDER_FAST_ABI_VERSION);
    if (p->width == 0 || p->height == 0 || (p->channels != 1 && p->channels != 3) ||
        (uint64_t)p->width * p->height > (uint64_t)INT32_MAX)
        return ffail(nullptr, ADDER_E_BAD_PARAMS, "plane %ux%ux%u", p->width, p->height, p->channels);
    if (p->threshold == 0)
        return ffail(nullptr, ADDER_E_BAD_PARAMS, "threshold 0 (1 .. 255: a score of 0 marks a pixel that is no corner)");
    if (p->nonmax > 1) return ffail(nullptr, ADDER_E_BAD_PARAMS, "nonmax %u (0 or 1)", p->nonmax);
    if (const int rc = api_check_device(p->device_id, g_fast_create_error)) return rc;
    AdderFast *f = new (std::nothrow) AdderFast();
    if (!f) return ffail(nullptr, ADDER_E_BAD_PARAMS, "out of host memory");
    f->p = *p;
    f->s = fast_shape(p->width, p->height, p->channels);
    if (hipSetDevice(p->device_id) != hipSuccess ||
        hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking) != hipSuccess ||
        hipMalloc((void **)&f->d_bad, sizeof(uint32_t)) != hipSuccess ||
        hipHostMalloc((void **)&f->h_bad, sizeof(uint32_t), hipHostMallocDefault) != hipSuccess) {
        fast_free(f);
        return ffail(nullptr, ADDER_E_HIP, "stream or flag allocation failed");
    }
    *out = f;
    return ADDER_OK;
}

extern "C" void adder_fast_destroy(AdderFast *f) { fast_free(f); }

extern "C" const char *adder_fast_last_error(const AdderFast *f) {
    return f ? f->err.c_str() : g_fast_create_error.c_str();
}

// every call waits for its results, so nothing of an earlier call still reads the scratch when it is replaced
static int ensure_sums(AdderFast *f, uint32_t n) {
    FHIPCHK(f, api_grow((void **)&f->d_sums, &f->d_sums_cap, (size_t)n * sizeof(FastFrameSums)));
    if (n > f->h_sums_frames) {
        if (f->h_sums) FHIPCHK(f, hipHostFree(f->h_sums));
        f->h_sums = nullptr;
        f->h_sums_frames = 0;
        FHIPCHK(f, hipHostMalloc((void **)&f->h_sums, (size_t)n * sizeof(FastFrameSums), hipHostMallocDefault));
        f->h_sums_frames = n;
    }
    return ADDER_OK;
}

// the detector into mask (and score), the counting against d_pred (may be null), the sums on the host
static int detect_and_count(AdderFast *f, const uint8_t *d_frames, const uint8_t *d_pred, uint32_t n, uint8_t *d_mask,
                            uint8_t *d_score, hipStream_t s) {
    const size_t planes = (size_t)n * f->s.plane;
    if (!d_mask) {
        FHIPCHK(f, api_grow((void **)&f->mask, &f->mask_cap, planes));
        d_mask = f->mask;
    }
    if (!d_score && f->p.nonmax) {
        FHIPCHK(f, api_grow((void **)&f->score, &f->score_cap, planes));
        d_score = f->score;
    }
    if (const int rc = ensure_sums(f, n)) return rc;
    FHIPCHK(f, fast_detect_run(f->s, d_frames, n, (int)f->p.threshold, f->p.nonmax != 0, d_mask, d_score, s));
    FHIPCHK(f, fast_count_run(f->s, d_mask, d_pred, n, f->d_sums, s));
    FHIPCHK(f, hipMemcpyAsync(f->h_sums, f->d_sums, (size_t)n * sizeof(FastFrameSums), hipMemcpyDeviceToHost, s));
    FHIPCHK(f, hipStreamSynchronize(s));
    return ADDER_OK;
}

static int detect(AdderFast *f, const uint8_t *d_frames, uint32_t n, uint8_t *d_mask, uint8_t *d_score, uint32_t *d_xy,
                  uint64_t capacity, uint64_t *counts, hipStream_t s) {
    if (!d_mask && d_xy) {  // the compaction reads the mask after the counts came back: the scratch plane
        FHIPCHK(f, api_grow((void **)&f->mask, &f->mask_cap, (size_t)n * f->s.plane));
        d_mask = f->mask;
    }
    if (const int rc = detect_and_count(f, d_frames, nullptr, n, d_mask, d_score, s)) return rc;
    uint64_t total = 0;
    for (uint32_t k = 0; k < n; ++k) total += (counts[k] = f->h_sums[k].gt);
    if (!d_xy) return ADDER_OK;
    if (total > capacity)
        return ffail(f, ADDER_E_OUT_CAPACITY, "coordinate list too small: %llu kept pixels, room for %llu",
                     (unsigned long long)total, (unsigned long long)capacity);
    if (total == 0u) return ADDER_OK;
    const uint32_t group = fast_group_frames(f->s);
    FHIPCHK(f, api_grow((void **)&f->offs, &f->offs_cap, (size_t)(n < group ? n : group) * f->s.plane * sizeof(uint32_t)));
    const size_t temp_bytes = fast_scan_temp_bytes(f->s, n);
    FHIPCHK(f, api_grow(&f->temp, &f->temp_cap, temp_bytes));
    FHIPCHK(f, fast_compact_run(f->s, d_mask, n, counts, f->offs, f->temp, temp_bytes, d_xy, capacity, s));
    FHIPCHK(f, hipStreamSynchronize(s));
    return ADDER_OK;
}

extern "C" int adder_fast_detect_device(AdderFast *f, const uint8_t *d_frames, uint32_t n_frames, uint8_t *d_mask,
                                        uint8_t *d_score, uint32_t *d_xy, uint64_t capacity, uint64_t *counts,
                                        void *stream) {
    if (!f) return ADDER_E_BAD_PARAMS;
    if (n_frames == 0) return ADDER_OK;
    if (!d_frames || !counts) return ffail(f, ADDER_E_BAD_PARAMS, "null pointer");
    FHIPCHK(f, hipSetDevice(f->p.device_id));
    return detect(f, d_frames, n_frames, d_mask, d_score, d_xy, capacity, counts, (hipStream_t)stream);
}

extern "C" int adder_fast_detect_host(AdderFast *f, const uint8_t *frames, uint32_t n_frames, uint8_t *mask,
                                      uint8_t *score, uint32_t *xy, uint64_t capacity, uint64_t *counts) {
    if (!f) return ADDER_E_BAD_PARAMS;
    if (n_frames == 0) return ADDER_OK;
    if (!frames || !counts) return ffail(f, ADDER_E_BAD_PARAMS, "null pointer");
    FHIPCHK(f, hipSetDevice(f->p.device_id));
    const size_t planes = (size_t)n_frames * f->s.plane;
    if (capacity > planes) capacity = planes;  // (a plane cannot keep more)
    FHIPCHK(f, api_stage_input(&f->d_in, &f->d_in_cap, frames, (size_t)n_frames * f->s.frame_bytes, f->stream));
    if (mask) FHIPCHK(f, api_grow((void **)&f->d_omask, &f->d_omask_cap, planes));
    if (score) FHIPCHK(f, api_grow((void **)&f->d_oscore, &f->d_oscore_cap, planes));
    if (xy) FHIPCHK(f, api_grow((void **)&f->d_oxy, &f->d_oxy_cap, (size_t)capacity * sizeof(uint32_t) + 4u));
    const int rc = detect(f, (const uint8_t *)f->d_in, n_frames, mask ? f->d_omask : nullptr,
                          score ? f->d_oscore : nullptr, xy ? f->d_oxy : nullptr, capacity, counts, f->stream);
    if (rc != ADDER_OK && rc != ADDER_E_OUT_CAPACITY) return rc;
    if (mask) FHIPCHK(f, hipMemcpy(mask, f->d_omask, planes, hipMemcpyDeviceToHost));
    if (score) FHIPCHK(f, hipMemcpy(score, f->d_oscore, planes, hipMemcpyDeviceToHost));
    if (xy && rc == ADDER_OK) {
        uint64_t total = 0;
        for (uint32_t k = 0; k < n_frames; ++k) total += counts[k];
        if (total) FHIPCHK(f, hipMemcpy(xy, f->d_oxy, (size_t)total * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    return rc;
}

extern "C" int adder_fast_mask_from_xy_device(AdderFast *f, const uint32_t *d_xy, uint64_t n, uint8_t *d_mask,
                                              void *stream) {
    if (!f) return ADDER_E_BAD_PARAMS;
    if (!d_mask || (!d_xy && n)) return ffail(f, ADDER_E_BAD_PARAMS, "null pointer");
    if (n > (uint64_t)INT32_MAX) return ffail(f, ADDER_E_BAD_PARAMS, "%llu coordinates", (unsigned long long)n);
    FHIPCHK(f, hipSetDevice(f->p.device_id));
    hipStream_t s = (hipStream_t)stream;
    if (n) {  // a list with a coordinate outside the plane is refused before the plane is touched
        FHIPCHK(f, hipMemsetAsync(f->d_bad, 0, sizeof(uint32_t), s));
        FHIPCHK(f, fast_xy_check_run(f->s, d_xy, n, f->d_bad, s));
        FHIPCHK(f, hipMemcpyAsync(f->h_bad, f->d_bad, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        FHIPCHK(f, hipStreamSynchronize(s));
        if (*f->h_bad)
            return ffail(f, ADDER_E_BAD_PARAMS, "a coordinate outside the %ux%u plane", f->s.width, f->s.height);
    }
    FHIPCHK(f, fast_xy_mask_run(f->s, d_xy, n, d_mask, s));
    return ADDER_OK;
}

static void fill_eval(const AdderFast *f, uint32_t n, AdderFastEval *out) {
    for (uint32_t k = 0; k < n; ++k) {
        const FastFrameSums &fs = f->h_sums[k];
        const FastConfusion c = fast_confusion_from(f->s.plane, fs.gt, fs.pred, fs.both);
        AdderFastEval e{};
        e.tp = c.tp;
        e.fp = c.fp;
        e.tn = c.tn;
        e.fn = c.fn;
        e.gt_count = fs.gt;
        e.pred_count = fs.pred;
        e.precision = c.precision;
        e.recall = c.recall;
        e.accuracy = c.accuracy;
        out[k] = e;
    }
}

extern "C" int adder_fast_evaluate_device(AdderFast *f, const uint8_t *d_frames, const uint8_t *d_prediction,
                                          uint32_t n_frames, AdderFastEval *out, void *stream) {
    if (!f) return ADDER_E_BAD_PARAMS;
    if (n_frames == 0) return ADDER_OK;
    if (!d_frames || !d_prediction || !out) return ffail(f, ADDER_E_BAD_PARAMS, "null pointer");
    FHIPCHK(f, hipSetDevice(f->p.device_id));
    if (const int rc = detect_and_count(f, d_frames, d_prediction, n_frames, nullptr, nullptr, (hipStream_t)stream))
        return rc;
    fill_eval(f, n_frames, out);
    return ADDER_OK;
}

extern "C" int adder_fast_evaluate_host(AdderFast *f, const uint8_t *frames, const uint8_t *prediction,
                                        uint32_t n_frames, AdderFastEval *out) {
    if (!f) return ADDER_E_BAD_PARAMS;
    if (n_frames == 0) return ADDER_OK;
    if (!frames || !prediction || !out) return ffail(f, ADDER_E_BAD_PARAMS, "null pointer");
    FHIPCHK(f, hipSetDevice(f->p.device_id));
    FHIPCHK(f, api_stage_input(&f->d_in, &f->d_in_cap, frames, (size_t)n_frames * f->s.frame_bytes, f->stream));
    FHIPCHK(f, api_stage_input(&f->d_pred, &f->d_pred_cap, prediction, (size_t)n_frames * f->s.plane, f->stream));
    if (const int rc = detect_and_count(f, (const uint8_t *)f->d_in, (const uint8_t *)f->d_pred, n_frames, nullptr,
                                        nullptr, f->stream))
        return rc;
    fill_eval(f, n_frames, out);
    return ADDER_OK;
}
