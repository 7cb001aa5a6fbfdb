// adder_fast_logic.hpp -- the per-pixel rules of the dense FAST 9_16 detector and of its scoring against a predicted
// feature set (include/adder_fast.h): the corner test with a threshold parameter, the corner score, strict
// 3x3 suppression, the confusion counts and the three ratios of feature_precision_recall_accuracy (utils/cv.rs:235-279).
// ADDER_HD: adder_fast.hip runs these on the device, plain g++ compiles the same text for tests/cpu_sim/fast_eval_sim.cpp
// and for the host column of tools/fast_eval_bench.py.  The plane-level loops at the end are host code.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "adder_pixel.hpp"  // ADDER_HD, fast_arc9, kFastBorder, kFastThreshold

namespace adder {

// cv.rs:25-30 CIRCLE3 as (dx, dy), nibble-packed with a +3 bias (the table fast9_is_feature walks)
constexpr uint64_t kFastRingDx = 0x2100012345666543ull, kFastRingDy = 0x6543210001234566ull;
ADDER_HD int fast_ring_dx(uint32_t k) { return (int)((kFastRingDx >> (4u * k)) & 0xfu) - 3; }
ADDER_HD int fast_ring_dy(uint32_t k) { return (int)((kFastRingDy >> (4u * k)) & 0xfu) - 3; }

// cv.rs:61 is_border(.., 3): the pixels the detector looks at
ADDER_HD bool fast_candidate(uint32_t w, uint32_t h, uint32_t x, uint32_t y) {
    return x >= kFastBorder && x + kFastBorder < w && y >= kFastBorder && y + kFastBorder < h;
}

// centre c, ring[k] in CIRCLE3 order: 9 circularly contiguous ring pixels all > c + threshold or all < c - threshold
ADDER_HD bool fast_corner(int c, const int (&ring)[16], int threshold) {
    uint32_t bright = 0u, dark = 0u;
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) {
        bright |= (ring[k] > c + threshold ? 1u : 0u) << k;
        dark |= (ring[k] < c - threshold ? 1u : 0u) << k;
    }
    return fast_arc9(bright) || fast_arc9(dark);
}

// Both directions of one ring position side by side: (ring - c, c - ring).  A type P with fast_pmin / fast_pmax /
// fast_phmax works in fast_score_from; the device's packs the two into one register as 16-bit halves.
struct FastPair {
    int b, d;
};
ADDER_HD FastPair fast_pair(int ring, int c, const FastPair *) { return FastPair{ring - c, c - ring}; }
ADDER_HD FastPair fast_pmin(FastPair x, FastPair y) { return FastPair{x.b < y.b ? x.b : y.b, x.d < y.d ? x.d : y.d}; }
ADDER_HD FastPair fast_pmax(FastPair x, FastPair y) { return FastPair{x.b > y.b ? x.b : y.b, x.d > y.d ? x.d : y.d}; }
ADDER_HD int fast_phmax(FastPair x) { return x.b > x.d ? x.b : x.d; }

// max over both directions and the 16 arcs of (min over the arc's 9 signed differences) - 1: the largest threshold at
// which the pixel is still a corner (at most 254; below the threshold in use exactly when the pixel is no corner there,
// negative when it is one at no threshold).
// The arc minima by doubling: runs of 2, 4, 8, then 9.
template <class P>
ADDER_HD int fast_score_from(int c, const int (&ring)[16]) {
    P v[16], m2[16], m4[16], m8[16];
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) v[k] = fast_pair(ring[k], c, (const P *)nullptr);
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) m2[k] = fast_pmin(v[k], v[(k + 1u) & 15u]);
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) m4[k] = fast_pmin(m2[k], m2[(k + 2u) & 15u]);
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) m8[k] = fast_pmin(m4[k], m4[(k + 4u) & 15u]);
    P best = fast_pmin(m8[0], v[8]);
#pragma unroll
    for (uint32_t k = 1; k < 16; ++k) best = fast_pmax(best, fast_pmin(m8[k], v[(k + 8u) & 15u]));
    return fast_phmax(best) - 1;
}

// the score byte of a candidate pixel: 0 for a non-corner, else threshold .. 254
template <class P>
ADDER_HD uint32_t fast_score_byte(int c, const int (&ring)[16], int threshold) {
    const int s = fast_score_from<P>(c, ring);
    return s >= threshold ? (uint32_t)s : 0u;
}

// nonmax: kept iff the score is strictly above each of the 8 neighbours' (a pixel outside the plane counts as 0)
ADDER_HD bool fast_nonmax_keep(uint32_t s, const uint32_t (&nb)[8]) {
    bool keep = s != 0u;
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) keep = keep && s > nb[k];
    return keep;
}

// 0x01 in every byte of v that is not zero
ADDER_HD uint32_t fast_nonzero_bytes(uint32_t v) {
    return ((((v & 0x7f7f7f7fu) + 0x7f7f7f7fu) | v) & 0x80808080u) >> 7;
}

// cv.rs:258-278 from the three sums a frame keeps: truth, predicted, both
struct FastConfusion {
    uint64_t tp, fp, tn, fn;
    double precision, recall, accuracy;  // the reference's f64 divisions; 0 / 0 stays NaN
};
inline FastConfusion fast_confusion_from(uint64_t positions, uint64_t gt, uint64_t pred, uint64_t both) {
    FastConfusion r;
    r.tp = both;
    r.fp = pred - both;
    r.fn = gt - both;
    r.tn = positions - r.tp - r.fp - r.fn;
    r.precision = (double)r.tp / (double)(r.tp + r.fp);
    r.recall = (double)r.tp / (double)(r.tp + r.fn);
    r.accuracy = (double)(r.tp + r.tn) / (double)(r.tp + r.tn + r.fp + r.fn);
    return r;
}

// ---- the same rules over a whole plane, on the host ----
// img [h][w][channels] (channel 0 looked at) -> score [h][w] (what the device's score plane holds)
inline void fast_score_plane_host(const uint8_t *img, uint32_t w, uint32_t h, uint32_t channels, int threshold,
                                  bool want_score, uint8_t *out) {
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = 0; x < w; ++x) {
            uint8_t v = 0;
            if (fast_candidate(w, h, x, y)) {
                const int c = (int)img[((size_t)y * w + x) * channels];
                int ring[16];
                for (uint32_t k = 0; k < 16; ++k)
                    ring[k] = (int)img[((size_t)((int)y + fast_ring_dy(k)) * w + (size_t)((int)x + fast_ring_dx(k))) * channels];
                if (fast_corner(c, ring, threshold)) v = want_score ? (uint8_t)fast_score_byte<FastPair>(c, ring, threshold) : 1u;
            }
            out[(size_t)y * w + x] = v;
        }
}

inline void fast_nonmax_plane_host(const uint8_t *score, uint32_t w, uint32_t h, uint8_t *mask) {
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = 0; x < w; ++x) {
            uint32_t nb[8], k = 0;
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    if (dx == 0 && dy == 0) continue;
                    const int xx = (int)x + dx, yy = (int)y + dy;
                    nb[k++] = (xx >= 0 && xx < (int)w && yy >= 0 && yy < (int)h) ? score[(size_t)yy * w + (size_t)xx] : 0u;
                }
            mask[(size_t)y * w + x] = fast_nonmax_keep(score[(size_t)y * w + x], nb) ? 1u : 0u;
        }
}

// One frame as adder_fast_detect does it: mask [h][w] (1 = kept) and score [h][w] (either may be null; `work` is
// 2 * h * w bytes of scratch).  Returns the number kept.
inline uint64_t fast_detect_plane_host(const uint8_t *img, uint32_t w, uint32_t h, uint32_t channels, int threshold,
                                       bool nonmax, uint8_t *mask, uint8_t *score, uint8_t *work) {
    const size_t n = (size_t)w * h;
    uint8_t *s = score ? score : work;
    uint8_t *m = mask ? mask : work + n;
    fast_score_plane_host(img, w, h, channels, threshold, nonmax || score, s);
    if (nonmax)
        fast_nonmax_plane_host(s, w, h, m);
    else
        for (size_t i = 0; i < n; ++i) m[i] = s[i] != 0u ? 1u : 0u;
    uint64_t kept = 0;
    for (size_t i = 0; i < n; ++i) kept += m[i];
    return kept;
}

// the kept pixels of a mask as x | y << 16, in raster order; returns their number (xy may be null: count only)
inline uint64_t fast_list_host(const uint8_t *mask, uint32_t w, uint32_t h, uint32_t *xy) {
    uint64_t n = 0;
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = 0; x < w; ++x)
            if (mask[(size_t)y * w + x]) {
                if (xy) xy[n] = x | (y << 16);
                ++n;
            }
    return n;
}

// truth [n] of 0 / 1 against pred [n] (nonzero = predicted), four bytes at a time as the device's kernel does
inline FastConfusion fast_confusion_host(const uint8_t *truth, const uint8_t *pred, uint64_t n) {
    uint64_t gt = 0, pr = 0, both = 0, i = 0;
    for (; i + 4u <= n; i += 4u) {
        uint32_t a, b;
        __builtin_memcpy(&a, truth + i, 4);
        __builtin_memcpy(&b, pred + i, 4);
        a = fast_nonzero_bytes(a);
        b = fast_nonzero_bytes(b);
        gt += (uint64_t)__builtin_popcount(a);
        pr += (uint64_t)__builtin_popcount(b);
        both += (uint64_t)__builtin_popcount(a & b);
    }
    for (; i < n; ++i) {
        const uint32_t a = truth[i] ? 1u : 0u, b = pred[i] ? 1u : 0u;
        gt += a;
        pr += b;
        both += a & b;
    }
    return fast_confusion_from(n, gt, pr, both);
}

}  // namespace adder
