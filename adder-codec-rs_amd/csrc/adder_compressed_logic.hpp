// adder_compressed_logic.hpp -- the compressed codec's source model as pure functions, for the host and the device
// alike (adder_compressed_model.hip runs them per lane, tests/cpu_sim/compressed_model_main.cpp runs them serially under
// plain g++).  A restatement of csrc/adder_compressed.cpp's compress_adu / pixel_lists / encoder_ingest with the same
// integer widths and casts; that file's own paths do not use this header and stay what they are.
//
// What the range coder consumes is a sequence of (context, fenwick index) pairs, so the model's whole output is a
// stream of 16-bit symbol words, context << 10 | index:
//   context 0 d (index <= 513), 1 t (byte + 1), 2 bitshift (shift + 1), 3 eof (index 0).
// Every emitting function is a template over a sink with put(uint16_t): CmCountSink counts, CmWriteSink stores, so the
// size of a pixel's or a cube's symbols and the symbols themselves come out of one body.
//
// f64: the lossy bit shift compares intensities (cabac_contexts.rs:75-150).  The device must produce the host's bits:
// no fast-math, an IEEE division, ldexp for 2^d, and no contraction -- inlined, `intensity * dt_ref` followed by
// `- c_thresh_max` would fuse into one fma.  The pragma below switches contraction off inside the functions that do
// the arithmetic, whatever the command line says (g++ has no such pragma: x86-64 builds of it do not contract without
// -mfma, and the tests' build passes -ffp-contract=off as well).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ADDER_CM_HD __host__ __device__ inline
#else
#define ADDER_CM_HD inline
#endif
#if defined(__clang__)
#define ADDER_CM_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define ADDER_CM_NO_CONTRACT
#endif

namespace adder {

constexpr uint32_t kCmBlock = 16;            // event_structure/mod.rs:8
constexpr int kCmNoEvent = 256;              // DRESIDUAL_NO_EVENT
constexpr int kCmSkipCube = 257;             // DRESIDUAL_SKIP_CUBE
constexpr int kCmDResidualOffset = 255;      // cabac_contexts.rs:21
constexpr uint32_t kCmEncodeFull = 15;       // BITSHIFT_ENCODE_FULL
constexpr uint32_t kCmDEmpty = 255;
constexpr int64_t kCmTResidualMax = (256 - 2) / 2;  // cabac_contexts.rs:33

// ---- the symbol word
enum : uint32_t { kCmCtxD = 0, kCmCtxT = 1, kCmCtxBitshift = 2, kCmCtxEof = 3 };
constexpr uint32_t kCmIndexBits = 10;
constexpr uint32_t kCmIndexMask = (1u << kCmIndexBits) - 1u;
// fenwick entries of a context's table (adder_compressed.cpp's Model): an index at or above it is no symbol
ADDER_CM_HD uint32_t cm_context_entries(uint32_t ctx) {
    return ctx == kCmCtxD ? 514u : ctx == kCmCtxT ? 257u : ctx == kCmCtxBitshift ? 17u : ctx == kCmCtxEof ? 2u : 0u;
}
ADDER_CM_HD uint16_t cm_symbol(uint32_t ctx, uint32_t index) { return (uint16_t)(ctx << kCmIndexBits | index); }
ADDER_CM_HD uint32_t cm_symbol_context(uint16_t w) { return (uint32_t)w >> kCmIndexBits; }
ADDER_CM_HD uint32_t cm_symbol_index(uint16_t w) { return (uint32_t)w & kCmIndexMask; }
ADDER_CM_HD bool cm_symbol_valid(uint16_t w) { return cm_symbol_index(w) < cm_context_entries(cm_symbol_context(w)); }
ADDER_CM_HD uint16_t cm_symbol_eof() { return cm_symbol(kCmCtxEof, 0u); }
ADDER_CM_HD uint16_t cm_symbol_no_event() { return cm_symbol(kCmCtxD, (uint32_t)(kCmNoEvent + kCmDResidualOffset) + 1u); }
ADDER_CM_HD uint16_t cm_symbol_skip_cube() { return cm_symbol(kCmCtxD, (uint32_t)(kCmSkipCube + kCmDResidualOffset) + 1u); }

struct CmCountSink {
    uint64_t n = 0;
    ADDER_CM_HD void put(uint16_t) { ++n; }
};
struct CmWriteSink {
    uint16_t *p;
    ADDER_CM_HD void put(uint16_t w) { *p++ = w; }
};

template <class S>
ADDER_CM_HD void cm_put_be16(S &s, uint32_t ctx, int16_t v) {  // ArithEncoder::bytes over be16
    s.put(cm_symbol(ctx, (uint32_t)((uint16_t)v >> 8) + 1u));
    s.put(cm_symbol(ctx, (uint32_t)((uint16_t)v & 0xffu) + 1u));
}
template <class S>
ADDER_CM_HD void cm_put_be64(S &s, uint32_t ctx, int64_t v) {
    for (int i = 0; i < 8; ++i) s.put(cm_symbol(ctx, (uint32_t)(((uint64_t)v >> (56 - 8 * i)) & 0xffu) + 1u));
}
template <class S>
ADDER_CM_HD void cm_put_start_t(S &s, uint32_t start_t) {  // the ADU's first four symbols
    for (int sh = 24; sh >= 0; sh -= 8) s.put(cm_symbol(kCmCtxT, ((start_t >> sh) & 0xffu) + 1u));
}

struct CmEv {  // EventCoordless
    uint32_t d, t;
};

struct CmParams {
    uint32_t dt_ref;         // ref_interval
    uint32_t num_intervals;  // adu_interval
    double c_thresh_max;
};

// ---- the f64 part (cabac_contexts.rs:75-85)
ADDER_CM_HD double cm_event_to_intensity(uint32_t d, uint32_t delta_t, uint32_t dt_ref) {
    ADDER_CM_NO_CONTRACT
    double intensity;
    if (d >= 129u)
        intensity = 0.0;
    else {
        const double shift = d == 128u ? 0.0 : ldexp(1.0, (int)d);  // D_SHIFT[d] as f64; D_SHIFT[128] == 0
        intensity = delta_t == 0u ? shift : shift / (double)delta_t;
    }
    return intensity * (double)dt_ref;
}

// cabac_contexts.rs:87-150: the lossy bit shift of an inter-coded t residual
ADDER_CM_HD void cm_residual_to_bitshift2(int64_t t_prediction, int64_t r, CmEv event, CmEv prev, uint32_t dt_ref,
                                          double c_thresh_max, uint32_t &bitshift_out, int64_t &residual_out) {
    ADDER_CM_NO_CONTRACT
    const int64_t ar = r < 0 ? -r : r;
    if (ar < kCmTResidualMax) {
        bitshift_out = 0;
        residual_out = r;
        return;
    }
    const uint32_t actual_dt = event.t > prev.t ? event.t - prev.t : 0u;
    const double actual = cm_event_to_intensity(event.d, actual_dt, dt_ref);
    double recon = actual;
    uint32_t bitshift = 0;
    int64_t tr = ar;
    for (;;) {
        const double lo = actual - c_thresh_max, hi = actual + c_thresh_max;
        if (tr > kCmTResidualMax && lo < recon && hi > recon) {
            tr >>= 1;
            bitshift += 1;
            const uint32_t recon_t = (uint32_t)(t_prediction + tr);
            if (recon_t < prev.t) break;
            recon = cm_event_to_intensity(event.d, recon_t - prev.t, dt_ref);
        } else {
            break;
        }
    }
    bitshift = bitshift ? bitshift - 1u : 0u;
    tr = ar >> bitshift;
    if (tr < kCmTResidualMax) {
        bitshift_out = bitshift;
        residual_out = r < 0 ? -tr : tr;
    } else {
        bitshift_out = kCmEncodeFull;
        residual_out = r;
    }
}

// event_cube.rs:83-118
ADDER_CM_HD uint32_t cm_generate_t_prediction(uint64_t idx, int d_residual, uint32_t last_delta_t, CmEv prev,
                                              uint32_t num_intervals, uint32_t dt_ref, uint32_t start_t) {
    if (idx == 1u) return start_t + last_delta_t;
    if (d_residual > 14 || d_residual < -14) d_residual = 0;
    if (prev.d == kCmDEmpty) d_residual = -1;
    const uint32_t pred =
        d_residual < 0 ? last_delta_t >> (uint32_t)(-d_residual) : last_delta_t << (uint32_t)d_residual;
    const uint32_t cap = (num_intervals & 0xffu) * dt_ref;
    const uint32_t step = pred < cap ? pred : cap;
    const uint32_t next = prev.t + step;
    return prev.t > next ? prev.t : next;
}

// ---- intra (compress_adu's first loop): the first kept event of a non-empty pixel.  `have_init`: an earlier pixel of
// the cube (c, y, x order) was non-empty, and `init` is that pixel's first event; without one the event is coded
// against (its own d, start_t).  Lossless: the decoder gets the event's own t back.  4 or 10 symbols.
// -> the bit shift symbol's value (0 or 15)
template <class S>
ADDER_CM_HD uint32_t cm_intra_pixel(S &s, bool have_init, CmEv init, CmEv event, uint32_t start_t) {
    if (have_init) {
        s.put(cm_symbol(kCmCtxD, (uint32_t)((int)event.d - (int)init.d + kCmDResidualOffset) + 1u));
    } else {
        s.put(cm_symbol(kCmCtxD, (uint32_t)((int)event.d + kCmDResidualOffset) + 1u));
        init = CmEv{event.d, start_t};
    }
    const int64_t r = (int64_t)event.t - (int64_t)init.t;
    const bool full = !((r < 0 ? -r : r) < kCmTResidualMax);  // residual_to_bitshift (:49-73)
    s.put(cm_symbol(kCmCtxBitshift, (full ? kCmEncodeFull : 0u) + 1u));
    if (full)
        cm_put_be64(s, kCmCtxT, r);
    else
        cm_put_be16(s, kCmCtxT, (int16_t)r);
    return full ? kCmEncodeFull : 0u;
}

// the drop rule of pixel_lists (event_cube.rs:135-151): with `kept` events already in the pixel's list, the last of
// them at (original) time last_t, is an event at time t dropped?
ADDER_CM_HD bool cm_ingest_drops(uint64_t kept, uint32_t last_t, uint32_t t) { return kept > 1u && t <= last_t; }

constexpr uint32_t kCmDropped = 16;  // the per-event code of a dropped event (0..15: the bit shift it was coded with)

// ---- inter (compress_adu's second loop) over one pixel's events of one ADU in arrival order, the drop rule applied
// on the way.  get(i) -> CmEv with the event's own t, i in [0, n), n >= 1; note(i, code, recon_t) is told every
// event's fate: code kCmDropped, or the bit shift of a kept one with the t the decoder gets back (event 0 is the intra
// event: the caller notes it).  The previous event of a kept one is the reconstructed one.  Emits each later kept
// event's symbols and the pixel's terminator.  -> the events kept (>= 1).
template <class S, class Get, class Note>
ADDER_CM_HD uint64_t cm_inter_pixel(S &s, Get get, uint64_t n, uint32_t start_t, const CmParams &p, Note note) {
    CmEv prev = get(0);        // reconstructed (intra is lossless)
    uint32_t last_t = prev.t;  // the last kept event's own t
    uint64_t kept = 1;
    uint32_t last_delta_t = 0;
    for (uint64_t i = 1; i < n; ++i) {
        CmEv event = get(i);
        if (cm_ingest_drops(kept, last_t, event.t)) {
            note(i, kCmDropped, 0u);
            continue;
        }
        last_t = event.t;
        const uint64_t idx = kept++;
        const int d_residual = (int)event.d - (int)prev.d;
        cm_put_be16(s, kCmCtxD, (int16_t)d_residual);
        const uint32_t t_pred =
            cm_generate_t_prediction(idx, d_residual, last_delta_t, prev, p.num_intervals, p.dt_ref, start_t);
        const int64_t r = (int64_t)event.t - (int64_t)t_pred;
        uint32_t bitshift;
        int64_t t_residual;
        cm_residual_to_bitshift2((int64_t)t_pred, r, event, prev, p.dt_ref, p.c_thresh_max, bitshift, t_residual);
        s.put(cm_symbol(kCmCtxBitshift, bitshift + 1u));
        if (bitshift == kCmEncodeFull) {
            cm_put_be64(s, kCmCtxT, t_residual);
            event.t = (uint32_t)((int64_t)t_pred + t_residual);
        } else {
            const int16_t tr = (int16_t)t_residual;
            cm_put_be16(s, kCmCtxT, tr);
            event.t = (uint32_t)((int64_t)t_pred + (int64_t)((uint64_t)(int64_t)tr << bitshift));
        }
        event.t = event.t > prev.t ? event.t : prev.t;
        last_delta_t = event.t - prev.t;
        note(i, bitshift, event.t);
        prev = event;
    }
    cm_put_be16(s, kCmCtxD, (int16_t)kCmNoEvent);
    return kept;
}

// ---- symbols of one ADU: 4 start_t bytes; one symbol per cube (a skip) with every non-skipped cube's grown to its
// npix pixels' and every non-empty pixel's to its 4 or 10; the inter symbols; eof.  64-bit throughout: a batch's
// offsets are sums of these.
ADDER_CM_HD uint64_t cm_adu_intra_symbols(uint64_t ncubes, uint64_t npix, uint64_t cubes_hit, uint64_t intra_extra) {
    return ncubes + cubes_hit * (npix - 1u) + intra_extra;
}
ADDER_CM_HD uint64_t cm_adu_symbols(uint64_t ncubes, uint64_t npix, uint64_t cubes_hit, uint64_t intra_extra,
                                    uint64_t inter) {
    return 4u + cm_adu_intra_symbols(ncubes, npix, cubes_hit, intra_extra) + inter + 1u;
}

// ---- the sort key of an event inside a call: (ADU within the call, cube row-major, c*256 + (y%16)*16 + x%16)
constexpr uint32_t kCmPixBits = 10;
ADDER_CM_HD uint32_t cm_pix_of(uint32_t x, uint32_t y, uint32_t c) {
    return c * 256u + (y % kCmBlock) * kCmBlock + x % kCmBlock;
}
ADDER_CM_HD uint64_t cm_key(uint64_t adu, uint64_t ncubes, uint32_t bx, uint32_t x, uint32_t y, uint32_t c) {
    const uint64_t cube = (uint64_t)(y / kCmBlock) * bx + x / kCmBlock;
    return ((adu * ncubes + cube) << kCmPixBits) | cm_pix_of(x, y, c);
}

// ---- the ADU cut (adder_compressed_encoder_ingest): an event with t > start_t + span closes the ADU, at most one ADU
// per event, u32 arithmetic.  The serial rule, and the blocked walk the device runs.
// -> the ADUs closed; adu_out[i] (may be null) = ADUs closed up to and including event i
ADDER_CM_HD uint64_t cm_cut_serial(const uint32_t *t, uint64_t n, uint32_t *start_t, uint32_t span, uint32_t *adu_out) {
    uint64_t k = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if (t[i] > (uint32_t)(*start_t + span)) {
            ++k;
            *start_t += span;
        }
        if (adu_out) adu_out[i] = (uint32_t)k;
    }
    return k;
}

// One block of up to 64 events.  gt(thr) -> the mask of the block's lanes whose t > thr (a ballot on the device).  Lanes
// behind each cut are tested again against the advanced start_t.  -> the mask of lanes that close an ADU; lane l's ADU
// is the block's first plus cm_cuts_upto(mask, l).
template <class Gt>
ADDER_CM_HD uint64_t cm_cut_block(Gt gt, uint32_t *start_t, uint32_t span) {
    uint64_t cuts = 0, open = ~0ull;  // open: the lanes not yet passed
    while (open) {
        const uint64_t m = gt((uint32_t)(*start_t + span)) & open;
        if (!m) break;
        const uint32_t f = (uint32_t)__builtin_ctzll(m);
        cuts |= 1ull << f;
        *start_t += span;
        open = f == 63u ? 0ull : ~0ull << (f + 1u);
    }
    return cuts;
}
ADDER_CM_HD uint32_t cm_popcount64(uint64_t v) { return (uint32_t)__builtin_popcountll(v); }
ADDER_CM_HD uint32_t cm_cuts_upto(uint64_t cuts, uint32_t lane) {
    return cm_popcount64(lane == 63u ? cuts : cuts & ((2ull << lane) - 1u));
}

// the walk over blocks of `lanes` (1..64) events as the device does it: a block whose maximum t does not pass the
// threshold is skipped whole.  Same outputs as cm_cut_serial.
inline uint64_t cm_cut_walk(const uint32_t *t, uint64_t n, uint32_t lanes, uint32_t *start_t, uint32_t span,
                            uint32_t *adu_out) {
    uint64_t k = 0;
    for (uint64_t b = 0; b < n; b += lanes) {
        const uint32_t m = n - b < lanes ? (uint32_t)(n - b) : lanes;
        uint32_t mx = 0;
        for (uint32_t l = 0; l < m; ++l) mx = t[b + l] > mx ? t[b + l] : mx;
        uint64_t cuts = 0;
        if (mx > (uint32_t)(*start_t + span)) {
            auto gt = [&](uint32_t thr) {
                uint64_t mask = 0;
                for (uint32_t l = 0; l < m; ++l) mask |= (uint64_t)(t[b + l] > thr) << l;
                return mask;
            };
            cuts = cm_cut_block(gt, start_t, span);
        }
        for (uint32_t l = 0; l < m && adu_out; ++l) adu_out[b + l] = (uint32_t)(k + cm_cuts_upto(cuts, l));
        k += cm_popcount64(cuts);
    }
    return k;
}

}  // namespace adder
