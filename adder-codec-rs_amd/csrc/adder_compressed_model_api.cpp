// adder_compressed_model_api.cpp -- C-ABI of the compressed codec's source model on the device
// (include/adder_compressed_model.h): argument checks, the buffers in HBM (the open ADU's events, the call
// scratch as one arena, the symbol and event outputs), the order of adder_compressed_model.hip's steps and the three
// places a call waits for a number the next step's sizes depend on (the ADUs closed, the runs, the totals).
// A call commits its state last, behind every step that can fail: a refusal (bad event, too little symbol room) or a
// failed HIP call leaves the object as it was.
#include <hip/hip_runtime.h>

#include <new>
#include <vector>

#include "../../include/adder_compressed_model.h"
#include "adder_api_util.hpp"
#include "adder_compressed_kernels.h"

using namespace adder;

static thread_local std::string g_cm_create_error;

struct AdderCompressedModel {
    AdderCompressedParams p{};
    int device_id = 0;
    CmShape sh{};
    hipStream_t stream = nullptr;  // close's stream
    uint32_t start_t = 0;          // of the open ADU
    bool closed = false;
    // the open ADU's events: work[cur][0 .. carry)
    AdderEvent *work[2] = {nullptr, nullptr};
    size_t work_cap[2] = {0, 0};  // bytes
    int cur = 0;
    uint64_t carry = 0;
    // call scratch
    void *arena = nullptr;
    size_t arena_cap = 0;
    uint64_t arena_events = 0;
    CmScratch s{};
    CmCutResult *h_res = nullptr;  // pinned
    // the device's share of a call: an event pair around each stretch of work between two host waits
    hipEvent_t span_ev[10] = {};
    int spans = 0;
    float device_ms = 0.0f;
    // outputs
    uint16_t *sym = nullptr;
    size_t sym_cap = 0;  // bytes
    AdderEvent *recon = nullptr;
    size_t recon_cap = 0;
    uint64_t sym_limit = 0, needed = 0;
    std::vector<uint32_t> adu_start;
    std::vector<uint64_t> sym_off, ev_off;  // n_adus + 1
    AdderCompressedModelCounters counters{};
    std::string err;
};

static int mfail(AdderCompressedModel *m, int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    api_fail(m ? m->err : g_cm_create_error, code, fmt, ap);
    va_end(ap);
    return code;
}
static int mfail(const AdderCompressedModel *m, int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    api_fail(m ? const_cast<AdderCompressedModel *>(m)->err : g_cm_create_error, code, fmt, ap);
    va_end(ap);
    return code;
}

#define MHIPCHK(m, expr) ADDER_HIPCHK(mfail, m, expr, #expr)

static void model_free(AdderCompressedModel *m) {
    if (!m) return;
    (void)hipSetDevice(m->device_id);
    (void)hipDeviceSynchronize();
    for (hipEvent_t e : m->span_ev)
        if (e) (void)hipEventDestroy(e);
    api_free_all({m->work[0], m->work[1], m->arena, m->sym, m->recon});
    if (m->h_res) (void)hipHostFree(m->h_res);
    if (m->stream) (void)hipStreamDestroy(m->stream);
    delete m;
}

namespace {
struct Carver {  // the arena's layout: sized with a null base, then carved
    char *base;
    size_t off = 0;
    template <typename T>
    T *take(uint64_t n) {
        off = (off + 255u) & ~(size_t)255u;
        T *r = base ? (T *)(base + off) : nullptr;
        off += (size_t)n * sizeof(T);
        return r;
    }
};
}  // namespace

static size_t carve(CmScratch &s, char *base, uint64_t e, size_t temp_bytes) {
    Carver c{base};
    const uint64_t chunks = e / kCmChunk + 1u, n1 = e + 2u;
    s.bmax = c.take<uint32_t>(chunks);
    s.bbad = c.take<uint32_t>(chunks);
    s.cstart = c.take<uint32_t>(chunks);
    s.cadu = c.take<uint32_t>(chunks);
    s.adu = c.take<uint32_t>(n1);
    s.keys0 = c.take<uint64_t>(n1);
    s.keys1 = c.take<uint64_t>(n1);
    s.vals0 = c.take<uint32_t>(n1);
    s.vals1 = c.take<uint32_t>(n1);
    s.sd = c.take<uint8_t>(n1);
    s.st = c.take<uint32_t>(n1);
    s.rt = c.take<uint32_t>(n1);
    s.code = c.take<uint8_t>(n1);
    s.phead = c.take<uint32_t>(n1);
    s.chead = c.take<uint32_t>(n1);
    s.pscan = c.take<uint32_t>(n1);
    s.cscan = c.take<uint32_t>(n1);
    s.kscan = c.take<uint32_t>(n1);
    s.prun_ev = c.take<uint32_t>(n1);
    s.crun_ev = c.take<uint32_t>(n1);
    s.intra_extra = c.take<uint32_t>(n1);
    s.inter_cnt = c.take<uint32_t>(n1);
    s.sx = c.take<uint64_t>(n1);
    s.si = c.take<uint64_t>(n1);
    s.adu_prun = c.take<uint32_t>(n1);  // a call of n events closes n ADUs at most
    s.adu_crun = c.take<uint32_t>(n1);
    s.adu_recon_off = c.take<uint64_t>(n1);
    s.adu_sym_cnt = c.take<uint64_t>(n1);
    s.adu_sym_off = c.take<uint64_t>(n1);
    s.hist_part = c.take<uint64_t>((uint64_t)kCmHistBlocks * kCmHistBins);
    s.res = c.take<CmCutResult>(1);
    s.temp = c.take<uint8_t>(temp_bytes);
    s.temp_bytes = temp_bytes;
    return c.off + 256u;
}

// scratch for a call over `events` events; nothing of an earlier call is in flight (every call waits for its results)
static int ensure_scratch(AdderCompressedModel *m, uint64_t events) {
    if (events <= m->arena_events && m->arena) return ADDER_OK;
    const uint64_t e = scratch_capacity(events);
    const size_t temp_bytes = cm_temp_bytes(e + 1u);
    CmScratch probe{};
    const size_t bytes = carve(probe, nullptr, e, temp_bytes);
    MHIPCHK(m, api_grow(&m->arena, &m->arena_cap, bytes));
    carve(m->s, (char *)m->arena, e, temp_bytes);
    m->arena_events = e;
    return ADDER_OK;
}

// work[which] holds room for `events`; the first `keep` events stay
static int ensure_work(AdderCompressedModel *m, int which, uint64_t events, uint64_t keep, hipStream_t stream) {
    const size_t bytes = (size_t)(events + 1u) * sizeof(AdderEvent);
    if (bytes <= m->work_cap[which]) return ADDER_OK;
    const size_t want = (size_t)(scratch_capacity(events) + 1u) * sizeof(AdderEvent);
    AdderEvent *fresh = nullptr;
    MHIPCHK(m, hipMalloc((void **)&fresh, want));
    if (keep) {
        hipError_t e = hipMemcpyAsync(fresh, m->work[which], (size_t)keep * sizeof(AdderEvent), hipMemcpyDeviceToDevice, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e != hipSuccess) {
            (void)hipFree(fresh);
            return mfail(m, ADDER_E_HIP, "copying the open ADU's events failed: %s", hipGetErrorString(e));
        }
    }
    if (m->work[which]) MHIPCHK(m, hipFree(m->work[which]));
    m->work[which] = fresh;
    m->work_cap[which] = want;
    return ADDER_OK;
}

// a stretch of device work between two host waits (five a call at most); the waits themselves are not in it
static hipError_t span_begin(AdderCompressedModel *m, hipStream_t stream) {
    return m->spans < 5 ? hipEventRecord(m->span_ev[2 * m->spans], stream) : hipSuccess;
}
static hipError_t span_end(AdderCompressedModel *m, hipStream_t stream) {
    if (m->spans >= 5) return hipSuccess;
    return hipEventRecord(m->span_ev[2 * m->spans++ + 1], stream);
}
// after the call's last wait: the spans' sum
static int spans_sum(AdderCompressedModel *m) {
    float sum = 0.0f;
    for (int i = 0; i < m->spans; ++i) {
        float ms = 0.0f;
        MHIPCHK(m, hipEventElapsedTime(&ms, m->span_ev[2 * i], m->span_ev[2 * i + 1]));
        sum += ms;
    }
    m->device_ms = sum;
    return ADDER_OK;
}

static void clear_results(AdderCompressedModel *m) {
    m->spans = 0;
    m->device_ms = 0.0f;
    m->adu_start.clear();
    m->sym_off.assign(1, 0);
    m->ev_off.assign(1, 0);
    m->needed = 0;
}

// ADUs 0 .. k-1 of work[cur][0 .. p), the first of them starting at start0; the first `carry` events are of ADU 0, the
// others have their number in s.adu.  Fills the outputs and the results, and leaves the histogram in h_res; commits
// nothing else (commit_counters, once the caller's own steps are through).
static int run_model(AdderCompressedModel *m, uint64_t p, uint64_t carry, uint32_t k, uint32_t start0,
                     hipStream_t stream) {
    const CmShape &sh = m->sh;
    if ((uint64_t)k * sh.ncubes > (1ull << 38))
        return mfail(m, ADDER_E_BAD_PARAMS, "%u ADUs of %llu cubes in one call: cut the call", k,
                     (unsigned long long)sh.ncubes);
    const uint64_t *keys = nullptr;
    MHIPCHK(m, span_begin(m, stream));
    MHIPCHK(m, cm_group(sh, m->work[m->cur], carry, p, k, m->s, &keys, stream));
    MHIPCHK(m, hipMemcpyAsync(m->h_res, m->s.res, sizeof(CmCutResult), hipMemcpyDeviceToHost, stream));
    MHIPCHK(m, span_end(m, stream));
    MHIPCHK(m, hipStreamSynchronize(stream));
    const uint64_t runs_pixel = m->h_res->runs_pixel, runs_cube = m->h_res->runs_cube;
    if (runs_cube * sh.channels > 0x7fffffffull)  // a block per (hit cube, channel) fills its empty pixels
        return mfail(m, ADDER_E_BAD_PARAMS, "%llu hit cubes of %u channels in one call: cut the call",
                     (unsigned long long)runs_cube, sh.channels);
    MHIPCHK(m, span_begin(m, stream));
    MHIPCHK(m, cm_count(sh, keys, p, runs_pixel, k, start0, m->s, stream));
    std::vector<uint64_t> sym_off((size_t)k + 1u), ev_off((size_t)k + 1u);
    MHIPCHK(m, hipMemcpyAsync(sym_off.data(), m->s.adu_sym_off, sym_off.size() * 8u, hipMemcpyDeviceToHost, stream));
    MHIPCHK(m, hipMemcpyAsync(ev_off.data(), m->s.adu_recon_off, ev_off.size() * 8u, hipMemcpyDeviceToHost, stream));
    MHIPCHK(m, span_end(m, stream));
    MHIPCHK(m, hipStreamSynchronize(stream));
    const uint64_t total_sym = sym_off[k], total_ev = ev_off[k];
    if (m->sym_limit && total_sym > m->sym_limit) {
        clear_results(m);
        m->needed = total_sym;
        return mfail(m, ADDER_E_OUT_CAPACITY, "the call's %u ADUs need %llu symbol words, the capacity is %llu", k,
                     (unsigned long long)total_sym, (unsigned long long)m->sym_limit);
    }
    MHIPCHK(m, api_grow((void **)&m->sym, &m->sym_cap, (size_t)(total_sym + 1u) * sizeof(uint16_t)));
    MHIPCHK(m, api_grow((void **)&m->recon, &m->recon_cap, (size_t)(total_ev + 1u) * sizeof(AdderEvent)));
    MHIPCHK(m, span_begin(m, stream));
    MHIPCHK(m, cm_write(sh, keys, p, runs_pixel, runs_cube, k, start0, m->s, m->sym, m->recon, stream));
    MHIPCHK(m, hipMemcpyAsync(m->h_res, m->s.res, sizeof(CmCutResult), hipMemcpyDeviceToHost, stream));
    MHIPCHK(m, span_end(m, stream));
    MHIPCHK(m, hipStreamSynchronize(stream));
    m->adu_start.resize(k);
    for (uint32_t a = 0; a < k; ++a) m->adu_start[a] = start0 + a * sh.span;
    m->sym_off.swap(sym_off);
    m->ev_off.swap(ev_off);
    m->needed = total_sym;
    return ADDER_OK;
}

// the last step of a call that modelled p events: nothing can fail behind it
static void commit_counters(AdderCompressedModel *m, uint64_t p) {
    m->counters.events_in += p;
    m->counters.events_dropped += m->h_res->hist[kCmDropped];
    for (int b = 0; b < 16; ++b) m->counters.bitshift[b] += m->h_res->hist[b];
}

extern "C" int adder_compressed_model_create(const AdderCompressedParams *p, int device_id, AdderCompressedModel **out) {
    if (!out) return mfail((AdderCompressedModel *)nullptr, ADDER_E_BAD_PARAMS, "out is null");
    *out = nullptr;
    AdderCompressedModel *none = nullptr;
    if (!p || p->abi_version != ADDER_COMPRESSED_ABI_VERSION) return mfail(none, ADDER_E_BAD_PARAMS, "bad params / abi_version");
    if (!p->width || !p->height || (p->channels != 1 && p->channels != 3)) return mfail(none, ADDER_E_BAD_PARAMS, "bad plane");
    if (!p->ref_interval || !p->adu_interval || !p->delta_t_max || p->codec_version > 3)
        return mfail(none, ADDER_E_BAD_PARAMS, "bad ref_interval / adu_interval / delta_t_max / codec_version");
    if (const int rc = api_check_device(device_id, g_cm_create_error)) return rc;
    AdderCompressedModel *m = new (std::nothrow) AdderCompressedModel();
    if (!m) return mfail(none, ADDER_E_HIP, "out of memory");
    m->p = *p;
    m->device_id = device_id;
    CmShape &sh = m->sh;
    sh.width = p->width;
    sh.height = p->height;
    sh.channels = p->channels;
    sh.bx = (p->width + kCmBlock - 1u) / kCmBlock;
    sh.by = (p->height + kCmBlock - 1u) / kCmBlock;
    sh.ncubes = (uint64_t)sh.bx * sh.by;
    sh.npix = p->channels * 256u;
    sh.span = p->ref_interval * p->adu_interval;
    sh.prm = CmParams{p->ref_interval, p->adu_interval, (double)p->c_thresh_max};
    clear_results(m);
    if (hipSetDevice(device_id) != hipSuccess || hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking) != hipSuccess ||
        hipHostMalloc((void **)&m->h_res, sizeof(CmCutResult), hipHostMallocDefault) != hipSuccess) {
        model_free(m);
        return mfail(none, ADDER_E_HIP, "stream or result allocation failed");
    }
    for (hipEvent_t &e : m->span_ev)
        if (hipEventCreate(&e) != hipSuccess) {
            model_free(m);
            return mfail(none, ADDER_E_HIP, "event allocation failed");
        }
    *out = m;
    return ADDER_OK;
}

extern "C" void adder_compressed_model_destroy(AdderCompressedModel *m) { model_free(m); }

extern "C" const char *adder_compressed_model_last_error(const AdderCompressedModel *m) {
    return m ? m->err.c_str() : g_cm_create_error.c_str();
}

extern "C" int adder_compressed_model_set_symbol_capacity(AdderCompressedModel *m, uint64_t words) {
    if (!m) return ADDER_E_BAD_PARAMS;
    m->sym_limit = words;
    return ADDER_OK;
}

extern "C" int adder_compressed_model_needed(const AdderCompressedModel *m, uint64_t *words) {
    if (!m || !words) return ADDER_E_BAD_PARAMS;
    *words = m->needed;
    return ADDER_OK;
}

extern "C" int adder_compressed_model_ingest_device(AdderCompressedModel *m, const AdderEvent *d_events, size_t n,
                                                    void *stream_) {
    if (!m || (!d_events && n)) return ADDER_E_BAD_PARAMS;
    if (m->closed) return mfail(m, ADDER_E_BAD_PARAMS, "the model is closed");
    hipStream_t stream = (hipStream_t)stream_;
    MHIPCHK(m, hipSetDevice(m->device_id));
    clear_results(m);
    if (n == 0) return ADDER_OK;
    const uint64_t total = m->carry + n;
    if (total >= (uint64_t)INT32_MAX - 1u)
        return mfail(m, ADDER_E_BAD_PARAMS, "%llu events in the open ADU and the call: the sort counts in int",
                     (unsigned long long)total);
    if (const int rc = ensure_work(m, m->cur, total, m->carry, stream)) return rc;
    if (const int rc = ensure_scratch(m, total)) return rc;
    AdderEvent *work = m->work[m->cur];
    MHIPCHK(m, span_begin(m, stream));
    MHIPCHK(m, hipMemcpyAsync(work + m->carry, d_events, n * sizeof(AdderEvent), hipMemcpyDeviceToDevice, stream));
    MHIPCHK(m, cm_cut(m->sh, work + m->carry, n, m->start_t, m->s, stream));
    MHIPCHK(m, hipMemcpyAsync(m->h_res, m->s.res, sizeof(CmCutResult), hipMemcpyDeviceToHost, stream));
    MHIPCHK(m, span_end(m, stream));
    MHIPCHK(m, hipStreamSynchronize(stream));
    if (m->h_res->bad) return mfail(m, ADDER_E_BAD_PARAMS, "event outside the plane or channel");
    const uint32_t k = m->h_res->k, next_start = m->h_res->start_t;
    if (k == 0) {  // everything joins the open ADU
        m->carry = total;
        return spans_sum(m);
    }
    const uint64_t p = m->carry + m->h_res->p_new;
    if (p > total) return mfail(m, ADDER_E_HIP, "the cut left no open ADU");
    // room for the open ADU's events in the other buffer first: nothing is allocated behind the model
    const uint64_t rest = total - p;
    if (const int rc = ensure_work(m, m->cur ^ 1, rest, 0, stream)) return rc;
    if (const int rc = run_model(m, p, m->carry, k, m->start_t, stream)) return rc;
    hipError_t e = span_begin(m, stream);
    if (e == hipSuccess && rest)
        e = hipMemcpyAsync(m->work[m->cur ^ 1], work + p, (size_t)rest * sizeof(AdderEvent), hipMemcpyDeviceToDevice, stream);
    if (e == hipSuccess) e = span_end(m, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess || spans_sum(m) != ADDER_OK) {  // the object stays as it was: no results of a call that failed
        clear_results(m);
        return mfail(m, ADDER_E_HIP, "moving the open ADU's events failed: %s", hipGetErrorString(e));
    }
    // commit
    commit_counters(m, p);
    m->cur ^= 1;
    m->carry = rest;
    m->start_t = next_start;
    return ADDER_OK;
}

extern "C" int adder_compressed_model_close(AdderCompressedModel *m) {
    if (!m) return ADDER_E_BAD_PARAMS;
    MHIPCHK(m, hipSetDevice(m->device_id));
    clear_results(m);
    if (m->closed) return ADDER_OK;
    if (m->carry) {
        if (const int rc = ensure_scratch(m, m->carry)) return rc;
        if (const int rc = run_model(m, m->carry, m->carry, 1u, m->start_t, m->stream)) return rc;
        if (const int rc = spans_sum(m)) {
            clear_results(m);
            return rc;
        }
        commit_counters(m, m->carry);
        m->start_t += m->sh.span;
        m->carry = 0;
    }
    m->closed = true;
    return ADDER_OK;
}

extern "C" int adder_compressed_model_adus(const AdderCompressedModel *m, uint32_t *n_adus) {
    if (!m || !n_adus) return ADDER_E_BAD_PARAMS;
    *n_adus = (uint32_t)m->adu_start.size();
    return ADDER_OK;
}

extern "C" int adder_compressed_model_adu_info(const AdderCompressedModel *m, uint32_t cap, uint32_t *start_t,
                                               uint64_t *symbol_offsets, uint64_t *event_offsets) {
    if (!m) return ADDER_E_BAD_PARAMS;
    const size_t k = m->adu_start.size();
    if (cap < k) return mfail(m, ADDER_E_OUT_CAPACITY, "%zu ADUs, room for %u", k, cap);
    for (size_t a = 0; a < k && start_t; ++a) start_t[a] = m->adu_start[a];
    for (size_t a = 0; a <= k; ++a) {
        if (symbol_offsets) symbol_offsets[a] = m->sym_off[a];
        if (event_offsets) event_offsets[a] = m->ev_off[a];
    }
    return ADDER_OK;
}

extern "C" int adder_compressed_model_symbols_device(const AdderCompressedModel *m, const uint16_t **d_symbols,
                                                     uint64_t *n) {
    if (!m) return ADDER_E_BAD_PARAMS;
    if (d_symbols) *d_symbols = m->sym;
    if (n) *n = m->sym_off.back();
    return ADDER_OK;
}

extern "C" int adder_compressed_model_symbols(AdderCompressedModel *m, uint16_t *out, uint64_t cap) {
    if (!m || (!out && cap)) return ADDER_E_BAD_PARAMS;
    const uint64_t n = m->sym_off.back();
    if (cap < n) return mfail(m, ADDER_E_OUT_CAPACITY, "%llu symbol words, room for %llu", (unsigned long long)n, (unsigned long long)cap);
    MHIPCHK(m, hipSetDevice(m->device_id));
    if (n) MHIPCHK(m, hipMemcpy(out, m->sym, (size_t)n * sizeof(uint16_t), hipMemcpyDefault));
    return ADDER_OK;
}

extern "C" int adder_compressed_model_events_device(const AdderCompressedModel *m, const AdderEvent **d_events,
                                                    uint64_t *n) {
    if (!m) return ADDER_E_BAD_PARAMS;
    if (d_events) *d_events = m->recon;
    if (n) *n = m->ev_off.back();
    return ADDER_OK;
}

extern "C" int adder_compressed_model_events(AdderCompressedModel *m, AdderEvent *out, uint64_t cap) {
    if (!m || (!out && cap)) return ADDER_E_BAD_PARAMS;
    const uint64_t n = m->ev_off.back();
    if (cap < n) return mfail(m, ADDER_E_OUT_CAPACITY, "%llu events, room for %llu", (unsigned long long)n, (unsigned long long)cap);
    MHIPCHK(m, hipSetDevice(m->device_id));
    if (n) MHIPCHK(m, hipMemcpy(out, m->recon, (size_t)n * sizeof(AdderEvent), hipMemcpyDefault));
    return ADDER_OK;
}

extern "C" int adder_compressed_model_counters(const AdderCompressedModel *m, AdderCompressedModelCounters *out) {
    if (!m || !out) return ADDER_E_BAD_PARAMS;
    *out = m->counters;
    return ADDER_OK;
}

extern "C" int adder_compressed_model_last_device_ms(const AdderCompressedModel *m, float *ms) {
    if (!m || !ms) return ADDER_E_BAD_PARAMS;
    *ms = m->device_ms;
    return ADDER_OK;
}

extern "C" int adder_compressed_model_open_adu(const AdderCompressedModel *m, uint64_t *n_events, uint32_t *start_t) {
    if (!m) return ADDER_E_BAD_PARAMS;
    if (n_events) *n_events = m->carry;
    if (start_t) *start_t = m->start_t;
    return ADDER_OK;
}
