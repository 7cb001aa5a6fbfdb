// g++ build of csrc/adder_fast_logic.hpp for tests/test_fast_eval_cpu.py: the same text adder_fast.hip compiles,
// driven over whole planes on the host.
#include <stdint.h>

#include <vector>

#include "adder_fast_logic.hpp"

using namespace adder;

extern "C" {

// one frame as adder_fast_detect: mask / score [h][w], xy room for w * h; returns the number kept
uint64_t fes_detect(const uint8_t *img, uint32_t w, uint32_t h, uint32_t channels, int threshold, int nonmax,
                    uint8_t *mask, uint8_t *score, uint32_t *xy) {
    std::vector<uint8_t> work(2u * (size_t)w * h);
    const uint64_t kept = fast_detect_plane_host(img, w, h, channels, threshold, nonmax != 0, mask, score, work.data());
    const uint64_t listed = fast_list_host(mask, w, h, xy);
    return kept == listed ? kept : ~0ull;
}

// the closed-form score of every candidate whatever the threshold says (negative: a corner at no threshold), 0 at the others
void fes_raw_score(const uint8_t *img, uint32_t w, uint32_t h, uint32_t channels, int32_t *out) {
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = 0; x < w; ++x) {
            int32_t v = 0;
            if (fast_candidate(w, h, x, y)) {
                int ring[16];
                for (uint32_t k = 0; k < 16; ++k)
                    ring[k] = img[((size_t)((int)y + fast_ring_dy(k)) * w + (size_t)((int)x + fast_ring_dx(k))) * channels];
                v = fast_score_from<FastPair>((int)img[((size_t)y * w + x) * channels], ring);
            }
            out[(size_t)y * w + x] = v;
        }
}

// the event detectors' test (adder_pixel.hpp fast9_is_feature, threshold 30) at every pixel
void fes_fast9_plane(const uint8_t *img, uint32_t w, uint32_t h, uint32_t channels, uint8_t *out) {
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = 0; x < w; ++x) out[(size_t)y * w + x] = fast9_is_feature(img, w, h, channels, x, y) ? 1u : 0u;
}

// out: tp, fp, tn, fn; ratios: precision, recall, accuracy
void fes_confusion(const uint8_t *truth, const uint8_t *pred, uint64_t n, uint64_t *out, double *ratios) {
    const FastConfusion c = fast_confusion_host(truth, pred, n);
    out[0] = c.tp;
    out[1] = c.fp;
    out[2] = c.tn;
    out[3] = c.fn;
    ratios[0] = c.precision;
    ratios[1] = c.recall;
    ratios[2] = c.accuracy;
}

// adder_fast_evaluate of one frame on the host: out: tp, fp, tn, fn, kept; ratios as above (tools/fast_eval_bench.py's
// host column; work: 2 * w * h bytes)
void fes_evaluate(const uint8_t *img, uint32_t w, uint32_t h, uint32_t channels, int threshold, int nonmax,
                  const uint8_t *pred, uint8_t *work, uint64_t *out, double *ratios) {
    const size_t n = (size_t)w * h;
    out[4] = fast_detect_plane_host(img, w, h, channels, threshold, nonmax != 0, nullptr, nullptr, work);
    fes_confusion(work + n, pred, n, out, ratios);
}

}  // extern "C"
