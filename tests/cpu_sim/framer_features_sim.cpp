// framer_features_sim.cpp -- the device's feature-detection logic (csrc/adder_framer_features.hpp) compiled for the
// host, in the shape of the kernels of csrc/adder_framer_features.hip: unit keys, a stable sort, a walk per run that
// leaves val8 / t_after, a candidate test per event in input order with a binary search per ring pixel, and the plane
// and the carried event committed afterwards.  Test helper (tests/framer_features_sim_py.py).
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <map>
#include <numeric>
#include <vector>

#include "adder_framer_features.hpp"

using namespace adder;

namespace {

struct Ev {
    uint16_t x, y;
    uint8_t c, d;
    uint16_t pad;
    uint32_t t;
};
struct Feature {
    uint64_t index;
    uint32_t t;
    uint16_t x, y;
};
struct Frame {
    std::vector<uint32_t> val;
    std::vector<uint8_t> has;
};

struct Sim {
    uint32_t w, h, ch, n_units;
    FramerConsts k;
    std::vector<FramerPx> px;
    std::vector<uint8_t> plane;
    std::map<int64_t, Frame> frames;
    int64_t frames_written = 0;
    bool detect = false;
    uint32_t carry_valid = 0, carry_t = 0;
};

}  // namespace

extern "C" {

void *ffs_new(uint32_t w, uint32_t h, uint32_t ch, uint32_t tpf, uint32_t ref_interval, uint32_t abs_t, uint32_t round_up,
              uint32_t view_mode, uint32_t source_type, float practical_d_max, uint32_t delta_t_max, uint32_t value_type) {
    Sim *s = new Sim();
    s->w = w;
    s->h = h;
    s->ch = ch;
    s->n_units = w * h * ch;
    s->k = framer_consts(tpf, ref_interval, abs_t, round_up, view_mode, source_type, practical_d_max, delta_t_max, value_type);
    FramerPx p0;
    p0.ts = 0;
    p0.lastf = -1;
    p0.lasti = 0;
    s->px.assign(s->n_units, p0);
    s->plane.assign(s->n_units, 0);
    return s;
}
void ffs_free(void *h) { delete static_cast<Sim *>(h); }
void ffs_detect(void *h, int on) { static_cast<Sim *>(h)->detect = on != 0; }
void ffs_reset_last_event(void *h) { static_cast<Sim *>(h)->carry_valid = 0; }
int64_t ffs_frames_written(void *h) { return static_cast<Sim *>(h)->frames_written; }
void ffs_plane(void *h, uint8_t *out) {
    Sim *s = static_cast<Sim *>(h);
    memcpy(out, s->plane.data(), s->n_units);
}

// returns the number of features written to out (room for n); -1: an event outside the plane
int64_t ffs_ingest(void *h, const Ev *ev, uint32_t n, uint64_t index_base, Feature *out) {
    Sim *s = static_cast<Sim *>(h);
    if (!n) return 0;
    // keys + stable sort
    std::vector<uint32_t> keys(n), idx(n);
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t c = ev[i].c == 0xffu ? 0u : ev[i].c;
        if (ev[i].x >= s->w || ev[i].y >= s->h || c >= s->ch) return -1;
        keys[i] = (ev[i].y * s->w + ev[i].x) * s->ch + c;
    }
    std::iota(idx.begin(), idx.end(), 0u);
    std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
    // walk
    std::vector<uint8_t> val8_sorted(n), val8_input(n);
    std::vector<uint32_t> t_after(n), run_lo(s->n_units, 0u), run_hi(s->n_units, 0u);
    for (uint32_t j0 = 0; j0 < n;) {
        const uint32_t u = keys[idx[j0]];
        FramerPx p = s->px[u];
        uint32_t j = j0;
        for (; j < n && keys[idx[j]] == u; ++j) {
            const Ev &e = ev[idx[j]];
            const FramerFeatureStep o = framer_feature_step(p, e.d, e.t, s->k);
            if (o.fills) {
                for (int64_t f = std::max<int64_t>((int64_t)o.from + 1, s->frames_written); f <= o.to; ++f) {
                    Frame &fr = s->frames[f];
                    if (fr.val.empty()) {
                        fr.val.assign(s->n_units, 0u);
                        fr.has.assign(s->n_units, 0u);
                    }
                    fr.val[u] = p.lasti;
                    fr.has[u] = 1u;
                }
            }
            val8_sorted[j] = (uint8_t)o.val8;
            val8_input[idx[j]] = (uint8_t)o.val8;
            t_after[idx[j]] = o.t_after;
        }
        s->px[u] = p;
        run_lo[u] = j0;
        run_hi[u] = j;
        j0 = j;
    }
    if (!s->detect) return 0;
    // candidates, in input order; the plane is the one carried into the call
    int64_t count = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const bool last_valid = i > 0u ? true : s->carry_valid != 0u;
        const uint32_t last_t = i > 0u ? t_after[i - 1u] : s->carry_t;
        const uint32_t x = ev[i].x, y = ev[i].y;
        if (!framer_feature_is_candidate(x, y, ev[i].c, ev[i].t, last_valid, last_t, s->w, s->h)) continue;
        const bool feature = fast9_ring_is_feature((int)val8_input[i], [&](uint32_t k) -> int {
            const uint32_t ru = ((uint32_t)((int)y + fast_ring_dy(k)) * s->w + (uint32_t)((int)x + fast_ring_dx(k))) * s->ch;
            return (int)framer_feature_value_before(idx.data(), val8_sorted.data(), run_lo[ru], run_hi[ru], i, s->plane[ru]);
        });
        if (feature) {
            Feature f;
            f.index = index_base + i;
            f.t = ev[i].t;
            f.x = ev[i].x;
            f.y = ev[i].y;
            out[count++] = f;
        }
    }
    // commit
    for (uint32_t j = 0; j < n; ++j)
        if (j + 1u == n || keys[idx[j + 1u]] != keys[idx[j]]) s->plane[keys[idx[j]]] = val8_sorted[j];
    s->carry_valid = 1u;
    s->carry_t = t_after[n - 1u];
    return count;
}

// frame `frames_written` as u32 values, pixels without a value 0; complete_only: 0 when it is not complete
int ffs_pop_frame(void *h, uint32_t *out, int complete_only) {
    Sim *s = static_cast<Sim *>(h);
    auto it = s->frames.find(s->frames_written);
    bool complete = it != s->frames.end();
    if (complete)
        for (uint8_t b : it->second.has) complete = complete && b;
    if (complete_only && !complete) return 0;
    for (uint32_t u = 0; u < s->n_units; ++u)
        out[u] = (it != s->frames.end() && it->second.has[u]) ? it->second.val[u] : 0u;
    if (it != s->frames.end()) s->frames.erase(it);
    s->frames_written += 1;
    return 1;
}

// fast9_ring16_is_feature on every interior pixel of a [h][w][ch] image (ring gathered from channel 0)
void ffs_fast9_ring16_plane(const uint8_t *img, uint32_t w, uint32_t h, uint32_t ch, uint8_t *out) {
    memset(out, 0, (size_t)w * h);
    for (uint32_t y = kFastBorder; y + kFastBorder < h; ++y)
        for (uint32_t x = kFastBorder; x + kFastBorder < w; ++x) {
            uint8_t r[16];
            for (uint32_t k = 0; k < 16; ++k)
                r[k] = img[((size_t)((int)y + fast_ring_dy(k)) * w + (size_t)((int)x + fast_ring_dx(k))) * ch];
            out[(size_t)y * w + x] = fast9_ring16_is_feature((int)img[((size_t)y * w + x) * ch], r) ? 1u : 0u;
        }
}

}  // extern "C"
