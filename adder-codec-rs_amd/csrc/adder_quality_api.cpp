// adder_quality_api.cpp -- C-ABI of the quality metrics (include/adder_quality.h): argument checks, the call scratch in
// HBM, the launches of adder_quality.hip, and the host-side end of cv.rs:306-360 (MSE from the exact sum, PSNR with the
// platform libm, the SSIM of a frame from its channels' sums).  No CPU fallback.
#include <hip/hip_runtime.h>

#include <cmath>
#include <limits>
#include <new>

#include "../../include/adder_quality.h"
#include "adder_api_util.hpp"
#include "adder_quality_kernels.h"

using namespace adder;

static thread_local std::string g_quality_create_error;

struct AdderQuality {
    AdderQualityParams p{};
    QualityShape s{};
    hipStream_t stream = nullptr;  // the host-pointer form's stream
    uint32_t cap = 0;              // frames the scratch below holds
    unsigned long long *sse_part = nullptr;
    double *ssim_part = nullptr;
    QualityFrameSums *d_sums = nullptr;
    QualityFrameSums *h_sums = nullptr;  // pinned
    // host-pointer form: both inputs, and the map
    uint8_t *d_in = nullptr;
    size_t d_in_cap = 0;
    double *d_map = nullptr;
    size_t d_map_cap = 0;
    std::string err;
};

static int qfail(AdderQuality *q, int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    api_fail(q ? q->err : g_quality_create_error, code, fmt, ap);
    va_end(ap);
    return code;
}

#define QHIPCHK(q, expr) ADDER_HIPCHK(qfail, q, expr, #expr)

static void free_scratch(AdderQuality *q) {
    api_free_all({q->sse_part, q->ssim_part, q->d_sums});
    if (q->h_sums) (void)hipHostFree(q->h_sums);
    q->sse_part = nullptr;
    q->ssim_part = nullptr;
    q->d_sums = nullptr;
    q->h_sums = nullptr;
    q->cap = 0;
}

static void quality_free(AdderQuality *q) {
    if (!q) return;
    (void)hipSetDevice(q->p.device_id);
    if (q->stream) (void)hipStreamSynchronize(q->stream);
    free_scratch(q);
    api_free_all({q->d_in, q->d_map});
    if (q->stream) (void)hipStreamDestroy(q->stream);
    delete q;
}

// every call waits for its results, so nothing of an earlier call still reads the scratch when it is replaced
static int ensure_scratch(AdderQuality *q, uint32_t n) {
    if (n <= q->cap) return ADDER_OK;
    free_scratch(q);
    const uint32_t c = n;
    const bool ssim = (q->p.metrics & ADDER_QUALITY_SSIM) && q->s.windows;
    QHIPCHK(q, hipMalloc((void **)&q->sse_part, (size_t)c * q->s.sse_blocks * sizeof(unsigned long long)));
    if (ssim)
        QHIPCHK(q, hipMalloc((void **)&q->ssim_part,
                             (size_t)c * q->s.channels * q->s.tiles_x * q->s.tiles_y * sizeof(double)));
    QHIPCHK(q, hipMalloc((void **)&q->d_sums, (size_t)c * sizeof(QualityFrameSums)));
    QHIPCHK(q, hipHostMalloc((void **)&q->h_sums, (size_t)c * sizeof(QualityFrameSums), hipHostMallocDefault));
    q->cap = c;
    return ADDER_OK;
}

// cv.rs:317-330 and 380-390 on the device's exact SSE and fixed-order window sums
static void fill_results(const AdderQuality *q, uint32_t n, AdderQualityResult *out) {
    const QualityShape &s = q->s;
    const uint32_t m = q->p.metrics;
    volatile double v255 = 255.0;  // (evaluated by the platform libm at run time, as the host mirror does)
    const double psnr_peak = 20.0 * std::log10((double)v255);
    for (uint32_t f = 0; f < n; ++f) {
        const QualityFrameSums &fs = q->h_sums[f];
        AdderQualityResult r{};
        double mse = (double)fs.sse / (double)s.frame_bytes;
        if (mse == 0.0) mse = 0.0000001;  // "Make sure that PSNR isn't undefined"
        if (m & ADDER_QUALITY_MSE) r.mse = mse;
        if (m & ADDER_QUALITY_PSNR) r.psnr = psnr_peak - 10.0 * std::log10(mse);
        if (m & ADDER_QUALITY_SSIM) {
            if (s.windows == 0) {
                r.ssim = std::numeric_limits<double>::quiet_NaN();  // 0 / 0 in the reference's release build
            } else {
                const double weights = 64.0 * (double)s.windows;  // sum of 64 over the windows: exact
                double scores = 0.0;
                for (uint32_t ch = 0; ch < s.channels; ++ch) scores += fs.ssim64[ch] / weights;
                r.ssim = (scores / (double)s.channels) * 100.0;
            }
        }
        r.present = m;
        out[f] = r;
    }
}

extern "C" int adder_quality_create(const AdderQualityParams *p, AdderQuality **out) {
    if (!p || !out) return qfail(nullptr, ADDER_E_BAD_PARAMS, "null argument");
    *out = nullptr;
    if (p->abi_version != ADDER_QUALITY_ABI_VERSION)
        return qfail(nullptr, ADDER_E_BAD_PARAMS, "abi_version %u, this library is %u", p->abi_version,
                     ADDER_QUALITY_ABI_VERSION);
    if (p->width == 0 || p->height == 0 || (p->channels != 1 && p->channels != 3))
        return qfail(nullptr, ADDER_E_BAD_PARAMS, "plane %ux%ux%u", p->width, p->height, p->channels);
    const uint32_t all = ADDER_QUALITY_MSE | ADDER_QUALITY_PSNR | ADDER_QUALITY_SSIM;
    if (p->metrics == 0 || (p->metrics & ~all) != 0)
        return qfail(nullptr, ADDER_E_BAD_PARAMS, "metrics mask 0x%x (MSE 1 | PSNR 2 | SSIM 4, not empty)", p->metrics);
    if (const int rc = api_check_device(p->device_id, g_quality_create_error)) return rc;
    AdderQuality *q = new (std::nothrow) AdderQuality();
    if (!q) return qfail(nullptr, ADDER_E_BAD_PARAMS, "out of host memory");
    q->p = *p;
    q->s = quality_shape(p->width, p->height, p->channels);
    if (hipSetDevice(p->device_id) != hipSuccess || hipStreamCreateWithFlags(&q->stream, hipStreamNonBlocking) != hipSuccess) {
        quality_free(q);
        return qfail(nullptr, ADDER_E_HIP, "stream creation failed");
    }
    *out = q;
    return ADDER_OK;
}

extern "C" void adder_quality_destroy(AdderQuality *q) { quality_free(q); }

extern "C" const char *adder_quality_last_error(const AdderQuality *q) {
    return q ? q->err.c_str() : g_quality_create_error.c_str();
}

extern "C" uint64_t adder_quality_map_elems(const AdderQuality *q, uint32_t n_frames) {
    return q ? (uint64_t)n_frames * q->s.channels * q->s.windows : 0u;
}

static int compute(AdderQuality *q, const uint8_t *d_a, const uint8_t *d_b, uint32_t n, AdderQualityResult *out,
                   double *d_map, hipStream_t s) {
    int rc = ensure_scratch(q, n);
    if (rc != ADDER_OK) return rc;
    const bool ssim = (q->p.metrics & ADDER_QUALITY_SSIM) != 0u;
    QHIPCHK(q, quality_run(q->s, d_a, d_b, n, ssim, d_map, q->sse_part, q->ssim_part, q->d_sums, s));
    QHIPCHK(q, hipMemcpyAsync(q->h_sums, q->d_sums, (size_t)n * sizeof(QualityFrameSums), hipMemcpyDeviceToHost, s));
    QHIPCHK(q, hipStreamSynchronize(s));
    fill_results(q, n, out);
    return ADDER_OK;
}

static int check_call(AdderQuality *q, const void *a, const void *b, uint32_t n, const AdderQualityResult *out,
                      const double *map) {
    if (n == 0) return ADDER_OK;
    if (!a || !b || !out) return qfail(q, ADDER_E_BAD_PARAMS, "null pointer");
    if (map && !(q->p.metrics & ADDER_QUALITY_SSIM))
        return qfail(q, ADDER_E_BAD_PARAMS, "an SSIM map needs ADDER_QUALITY_SSIM in the metrics mask");
    return ADDER_OK;
}

extern "C" int adder_quality_compute_device(AdderQuality *q, const uint8_t *d_original, const uint8_t *d_reconstructed,
                                            uint32_t n_frames, AdderQualityResult *out, double *d_ssim_map,
                                            void *stream) {
    if (!q) return ADDER_E_BAD_PARAMS;
    int rc = check_call(q, d_original, d_reconstructed, n_frames, out, d_ssim_map);
    if (rc != ADDER_OK || n_frames == 0) return rc;
    QHIPCHK(q, hipSetDevice(q->p.device_id));
    return compute(q, d_original, d_reconstructed, n_frames, out, d_ssim_map, (hipStream_t)stream);
}

extern "C" int adder_quality_compute_host(AdderQuality *q, const uint8_t *original, const uint8_t *reconstructed,
                                          uint32_t n_frames, AdderQualityResult *out, double *ssim_map) {
    if (!q) return ADDER_E_BAD_PARAMS;
    int rc = check_call(q, original, reconstructed, n_frames, out, ssim_map);
    if (rc != ADDER_OK || n_frames == 0) return rc;
    QHIPCHK(q, hipSetDevice(q->p.device_id));
    const size_t bytes = (size_t)n_frames * q->s.frame_bytes;
    QHIPCHK(q, api_grow((void **)&q->d_in, &q->d_in_cap, 2 * bytes));
    const size_t map_elems = ssim_map ? (size_t)adder_quality_map_elems(q, n_frames) : 0u;
    if (map_elems) QHIPCHK(q, api_grow((void **)&q->d_map, &q->d_map_cap, map_elems * sizeof(double)));
    QHIPCHK(q, hipMemcpyAsync(q->d_in, original, bytes, hipMemcpyHostToDevice, q->stream));
    QHIPCHK(q, hipMemcpyAsync(q->d_in + bytes, reconstructed, bytes, hipMemcpyHostToDevice, q->stream));
    rc = compute(q, q->d_in, q->d_in + bytes, n_frames, out, map_elems ? q->d_map : nullptr, q->stream);
    if (rc != ADDER_OK) return rc;
    if (map_elems)
        QHIPCHK(q, hipMemcpy(ssim_map, q->d_map, map_elems * sizeof(double), hipMemcpyDeviceToHost));
    return ADDER_OK;
}
