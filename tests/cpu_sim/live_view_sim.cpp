// g++ build of the live view's two ADDER_HD decisions (adder-codec-rs_amd/csrc/adder_pixel.hpp): the byte a unit of the
// running-intensities plane gets in a view (view_value_u8) and "is this byte under a cross" (display_under_cross), for
// tests/test_live_view_cpu.py.
#include <stddef.h>
#include <stdint.h>

#include "adder_pixel.hpp"

using namespace adder;

extern "C" {
// out[i] = view_value_u8(d[i], t[i], clock[i], prev[i]) for one set of constants
void lvs_values(uint32_t view, uint32_t ref_time, uint32_t delta_t_max, float practical_d_max, const uint32_t *d,
                const uint32_t *t, const uint32_t *clock, const uint32_t *prev, size_t n, uint8_t *out) {
    const ViewConsts k{view, ref_time, delta_t_max, practical_d_max};
    for (size_t i = 0; i < n; ++i) out[i] = (uint8_t)view_value_u8(d[i], t[i], clock[i], prev[i], k);
}

struct PlaneMember {
    const uint8_t *m;
    uint32_t w;
    bool operator()(uint32_t x, uint32_t y) const { return m[(size_t)y * w + x] != 0u; }
};
// the display frame of `plane` ([h][w][channels]) with a cross on every member of m ([h][w]), by the gather
void lvs_display(const uint8_t *plane, const uint8_t *m, uint32_t w, uint32_t h, uint32_t channels, uint8_t *out) {
    const PlaneMember pm{m, w};
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = 0; x < w; ++x)
            for (uint32_t c = 0; c < channels; ++c) {
                const size_t i = ((size_t)y * w + x) * channels + c;
                out[i] = (display_drawn_channel(c, channels) && display_under_cross(pm, w, h, x, y)) ? (uint8_t)255u : plane[i];
            }
}
}
