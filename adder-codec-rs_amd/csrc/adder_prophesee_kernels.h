// adder_prophesee_kernels.h -- between adder_prophesee_api.cpp and adder_prophesee.hip (include/adder_prophesee.h is
// the public side).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "adder_chain_kernels.h"

namespace adder {

struct PphScalars {  // device words of one call, read back once
    unsigned long long bad;    // smallest record index outside the plane (UINT64_MAX: none)
    unsigned long long steps;  // sparse steps the records make
    unsigned long long end_bad;  // end_events: pixels whose last t equals running_t
};

struct PphArgs {
    uint32_t width, height, units;
    uint32_t key_bits;  // radix bits of a pixel key; key `units` marks a record outside the plane
    uint32_t ref_time;
    double theta;       // camera_theta, 0.02
    double ln_mid;      // ln_1p(128 / 255), the mid_clamp_u8 reset
    // per-pixel camera state: `cur` is read, a push's walk writes `nxt`, the commit copies the walked pixels back
    uint32_t *cur_t, *nxt_t;
    double *cur_ln, *nxt_ln;
};

struct PphScratch {
    ChainScratch chain;  // per push; cnt, offs and stage in input order
    PphScalars *sc;
};

// keys, sort by pixel, walk every pixel's run, scan the step counts; sc->bad and sc->steps are valid afterwards
hipError_t pph_generate(const PphArgs &a, const uint8_t *d_records, uint64_t n, const PphScratch &s, hipStream_t stream);
// places the steps in record order into d_steps and commits the walked pixels' state
hipError_t pph_emit(const PphArgs &a, uint64_t n, const PphScratch &s, AdderSparseStep *d_steps, hipStream_t stream);
// end_events: one step per pixel in raster order into d_steps; sc->end_bad counts the pixels that fail the assert
hipError_t pph_end_steps(const PphArgs &a, uint32_t running_t, AdderSparseStep *d_steps, PphScalars *sc,
                         hipStream_t stream);
// every pixel: last t = 2, last ln = ln_1p(128 / 255)
hipError_t pph_init_state(const PphArgs &a, hipStream_t stream);
// the records' t into a packed array (for the host's group scan)
hipError_t pph_times(const uint8_t *d_records, uint64_t n, uint32_t *d_t, hipStream_t stream);
hipError_t pph_exp_run(const double *d_x, double *d_y, uint64_t n, hipStream_t stream);

}  // namespace adder
