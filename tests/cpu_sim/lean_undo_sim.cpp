// tests/cpu_sim/lean_undo_sim.cpp -- TEST HARNESS, not product code.
//
// adder_lp_restore_kernel's arithmetic on the CPU: the device header's lr_unpack and lr_pack (adder_pixel.hpp, built by
// g++) over planes of header words and delta_t values.  tests/test_lean_undo_cpu.py holds them against the oracle's arenas.
#include <stddef.h>
#include <stdint.h>

#include "adder_pixel.hpp"

using namespace adder;

// (hdr, dt)[n] -> the four resident planes as lr_pack writes them; ok[u] = lr_unpack's consistency verdict
extern "C" void lean_undo_repack(const uint32_t *hdr, const float *dt, size_t n, float T, uint32_t *hdr_out, float *integ_out,
                                 float *dt_out, float *bdt_out, uint8_t *ok) {
    for (size_t u = 0; u < n; ++u) {
        bool consistent;
        const LrPx p = lr_unpack<ScalarLanes>(hdr[u], dt[u], T, consistent);
        hdr_out[u] = lr_pack<ScalarLanes>(p, T, integ_out[u], dt_out[u], bdt_out[u]);
        ok[u] = consistent ? 1 : 0;
    }
}

// the header word of a unit: base_val, the root's best d, fired levels, popped_dtm
extern "C" uint32_t lean_undo_hdr(uint32_t base, uint32_t bd, uint32_t m, int popped) { return hdr_make(base, bd, m, popped != 0); }
