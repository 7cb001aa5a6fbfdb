// adder_source_util.hpp -- what the camera sources' *_api.cpp (Prophesee, DAVIS) do alike around their own work: the
// push scratch of the shared chain (adder_chain_kernels.h), the step buffer, and the inner context their steps go to.
// Header-only free functions and plain structs, as adder_api_util.hpp: a context stays the struct its file declares.
#pragma once
#include "adder_api_util.hpp"
#include "adder_chain_kernels.h"

namespace adder {

inline void chain_free(ChainScratch &s) {
    api_free_all({s.keys0, s.keys1, s.idx0, s.idx1, s.cnt, s.offs, s.stage, s.temp});
    s = ChainScratch{};
}

// room for n records, and temp for them and for a scan over n_plane (0: none).  temp is there after the first call
// even when no record ever came: a DAVIS push with empty lists still scans its plane.
inline hipError_t chain_reserve(ChainScratch &s, uint64_t n, uint32_t n_plane) {
    hipError_t e = hipSuccess;
    auto mk = [&](void **b, size_t bytes) {
        if (e == hipSuccess) e = hipMalloc(b, bytes);
    };
    if (n > s.cap) {
        chain_free(s);
        const uint64_t c = scratch_capacity(n);
        for (uint32_t **b : {&s.keys0, &s.keys1, &s.idx0, &s.idx1, &s.cnt, &s.offs}) mk((void **)b, c * 4u);
        mk((void **)&s.stage, c * 2u * sizeof(AdderSparseStep));
        if (e != hipSuccess) return e;  // cap stays 0: the next call frees what was made
        s.cap = c;
    }
    if (!s.temp) {
        const size_t bytes = chain_temp_bytes(s.cap, n_plane);
        mk(&s.temp, bytes);
        if (e == hipSuccess) s.temp_bytes = bytes;
    }
    return e;
}

struct StepBuffer {  // the sparse steps a call hands to the inner context
    AdderSparseStep *p = nullptr;
    size_t bytes = 0;
};

inline hipError_t steps_reserve(StepBuffer &b, uint64_t n) {
    return api_grow((void **)&b.p, &b.bytes, n * sizeof(AdderSparseStep));
}

// (Re)opens a source's inner context: AbsoluteT, Collapse, running intensities on, the rest as the caller filled hp.
// limits_row: the Crf row that sets c_thresh_max and c_increase_velocity; baseline_row: the row whose baseline goes to
// reset_c_thresh; -1 leaves either alone.  *eps: the events one sparse step can make at most.  A failure's text is in
// err and *ctx is null or a context only reset helps.
inline int source_open_ctx(AdderHipCtx **ctx, AdderHipParams hp, int limits_row, int baseline_row, uint32_t units,
                           uint64_t *eps, std::string &err) {
    if (*ctx) adder_hip_destroy(*ctx);
    *ctx = nullptr;
    hp.time_mode = ADDER_TIME_ABSOLUTE_T;
    hp.multi_mode = ADDER_MULTI_COLLAPSE;
    if (limits_row >= 0) {
        hp.c_thresh_max = kCrf[limits_row][kCrfMax];
        hp.c_increase_velocity = kCrf[limits_row][kCrfVelocity];
    }
    int rc = adder_hip_create(&hp, ctx);
    if (rc != ADDER_OK) {
        *ctx = nullptr;
        err = std::string("inner context: ") + adder_hip_last_error(nullptr);
        return rc;
    }
    if (baseline_row >= 0 && (rc = adder_hip_reset_c_thresh(*ctx, kCrf[baseline_row][kCrfBaseline])) != ADDER_OK) {
        err = std::string("reset_c_thresh: ") + adder_hip_last_error(*ctx);
        return rc;
    }
    if ((rc = adder_hip_enable_running_intensities(*ctx, 1)) != ADDER_OK) {
        err = std::string("enable_running_intensities: ") + adder_hip_last_error(*ctx);
        return rc;
    }
    // a Continuous context bounds a frame at units * (max_depth + 3) events: the sparse integrator's bound per step
    *eps = adder_hip_max_events_per_frame(*ctx) / units;
    return ADDER_OK;
}

}  // namespace adder
