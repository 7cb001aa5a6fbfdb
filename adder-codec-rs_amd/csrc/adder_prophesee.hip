// adder_prophesee.hip -- Prophesee .dat records -> sparse steps on the device (include/adder_prophesee.h;
// prophesee.rs:174-258 and :325-365).
//
// The shape of adder_dvs.hip: a pixel's records form a serial chain, pixels are independent.
//   1. keys: decode each 8-byte record in place, pixel index as key (records outside the plane noted with atomicMin
//      and sorted behind every pixel); a stable radix sort brings a pixel's records together in camera order;
//   2. walk: a thread per run chains the pixel's last t and log intensity and writes each record's zero, one or two
//      steps into the record's two slots (input order), exps evaluated on the chain;
//   3. an exclusive scan of the step counts in input order places the steps, a thread per record copies them
//      (the sort, the scan and the copy are adder_chain.hip's, shared with adder_davis.hip);
//   4. commit: the walked pixels' state is copied back -- only after the host has checked the bad-record word and
//      the output room, so a refused push changes nothing.
// The steps then go to adder_hip_integrate_sparse_device unchanged.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "adder_exp.hpp"
#include "adder_prophesee_kernels.h"

namespace adder {

struct PphRec {
    uint32_t t, x, y, p;
};

// decode_event (prophesee.rs:437-452): x keeps 10 bits only, y is bits 14..27, p bit 28
__device__ __forceinline__ PphRec pph_load(const uint8_t *rec, uint64_t i) {
    const uint2 r = ((const uint2 *)rec)[i];
    PphRec e;
    e.t = r.x;
    e.x = r.y & 0x3ffu;
    e.y = (r.y & 0xfffc000u) >> 14;
    e.p = (r.y >> 28) & 1u;
    return e;
}

__device__ __forceinline__ uint8_t pph_as_u8(double v) { return !(v > 0.0) ? 0u : (v >= 255.0 ? 255u : (uint8_t)v); }

__device__ __forceinline__ AdderSparseStep pph_step(uint32_t x, uint32_t y, double val, float intensity, float time,
                                                    uint16_t flags) {
    AdderSparseStep s;
    s.x = (uint16_t)x;
    s.y = (uint16_t)y;
    s.c = 0xffu;
    s.frame_val = pph_as_u8(val);
    s.pad = flags;
    s.intensity = intensity;
    s.time = time;
    return s;
}

__global__ void pph_init_scalars_kernel(PphScalars *sc) {
    sc->bad = ~0ull;
    sc->steps = 0ull;
    sc->end_bad = 0ull;
}

__global__ __launch_bounds__(256) void pph_keys_kernel(const uint8_t *__restrict__ rec, uint64_t n, PphArgs a,
                                                       uint32_t *__restrict__ keys, uint32_t *__restrict__ idx,
                                                       PphScalars *sc) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const PphRec e = pph_load(rec, i);
    uint32_t key = a.units;
    if (e.x < a.width && e.y < a.height)
        key = e.y * a.width + e.x;
    else
        atomicMin(&sc->bad, (unsigned long long)i);
    keys[i] = key;
    idx[i] = (uint32_t)i;
}

// prophesee.rs:174-258 per pixel, in the mirror's order of operations
__global__ __launch_bounds__(256) void pph_walk_kernel(const uint8_t *__restrict__ rec, uint64_t n, PphArgs a,
                                                       const uint32_t *__restrict__ keys,
                                                       const uint32_t *__restrict__ idx, uint32_t *__restrict__ cnt,
                                                       AdderSparseStep *__restrict__ stage) {
    const uint64_t j0 = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j0 >= n) return;
    const uint32_t u = keys[j0];
    if (u >= a.units) {  // outside the plane: the push is refused, but every count is defined
        cnt[idx[j0]] = 0u;
        return;
    }
    if (j0 > 0u && keys[j0 - 1] == u) return;  // a thread per run of one pixel
    uint32_t lt = a.cur_t[u];
    double ln = a.cur_ln[u];
    const float ref_f = (float)a.ref_time;
    for (uint64_t j = j0; j < n && keys[j] == u; ++j) {
        const uint32_t i = idx[j];
        const PphRec e = pph_load(rec, i);
        const uint32_t t = e.t;
        if (t < lt) {  // :186-189
            cnt[i] = 0u;
            continue;
        }
        uint32_t c = 0u;
        AdderSparseStep *st = stage + 2u * (uint64_t)i;
        if (t > lt + 1u) {  // :196-217, u32 wrapping as the release build
            double v = (adder_exp(ln) - 1.0) * 255.0;
            if (v < 0.0 || v > 255.0) {  // mid_clamp_u8
                v = 128.0;
                ln = a.ln_mid;
            }
            const uint32_t gap = t - lt - 1u;
            st[c++] = pph_step(e.x, e.y, v, (float)(v * (double)gap), (float)(gap * a.ref_time), ADDER_SPARSE_NO_SIDE);
        }
        ln = e.p == 0u ? ln - a.theta : ln + a.theta;  // :220-227
        if (t > lt) {  // :232-255
            double v = (adder_exp(ln) - 1.0) * 255.0;
            if (v < 0.0 || v > 255.0) {
                v = 128.0;
                ln = a.ln_mid;
            }
            st[c++] = pph_step(e.x, e.y, v, (float)v, ref_f, 0u);
        }
        lt = t;
        cnt[i] = c;
    }
    a.nxt_t[u] = lt;
    a.nxt_ln[u] = ln;
}

__global__ __launch_bounds__(256) void pph_commit_kernel(uint64_t n, PphArgs a, const uint32_t *__restrict__ keys) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j >= n) return;
    const uint32_t u = keys[j];
    if (u >= a.units || (j > 0u && keys[j - 1] == u)) return;
    a.cur_t[u] = a.nxt_t[u];
    a.cur_ln[u] = a.nxt_ln[u];
}

// end_events (prophesee.rs:325-365): no clamp, time = (running_t - last_t) * ref_time, intensity = val * time
__global__ __launch_bounds__(256) void pph_end_kernel(PphArgs a, uint32_t running_t, AdderSparseStep *__restrict__ steps,
                                                      PphScalars *sc) {
    const uint32_t u = blockIdx.x * 256u + threadIdx.x;
    if (u >= a.units) return;
    const uint32_t d = running_t - a.cur_t[u];
    if (d == 0u) atomicAdd(&sc->end_bad, 1ull);  // assert!(running_t - last_t > 0)
    const double v = (adder_exp(a.cur_ln[u]) - 1.0) * 255.0;
    const uint32_t span = d * a.ref_time;
    steps[u] = pph_step(u % a.width, u / a.width, v, (float)(v * (double)span), (float)span, ADDER_SPARSE_NO_SIDE);
}

__global__ __launch_bounds__(256) void pph_init_state_kernel(PphArgs a) {
    const uint32_t u = blockIdx.x * 256u + threadIdx.x;
    if (u >= a.units) return;
    a.cur_t[u] = 2u;
    a.cur_ln[u] = a.ln_mid;
}

__global__ __launch_bounds__(256) void pph_times_kernel(const uint8_t *__restrict__ rec, uint64_t n,
                                                        uint32_t *__restrict__ t) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i < n) t[i] = ((const uint2 *)rec)[i].x;
}

__global__ __launch_bounds__(256) void pph_exp_kernel(const double *__restrict__ x, double *__restrict__ y, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i < n) y[i] = adder_exp(x[i]);
}

hipError_t pph_generate(const PphArgs &a, const uint8_t *rec, uint64_t n, const PphScratch &s, hipStream_t stream) {
    hipLaunchKernelGGL(pph_init_scalars_kernel, dim3(1), dim3(1), 0, stream, s.sc);
    if (n == 0u) return hipGetLastError();
    const uint32_t grid = grid_of(n);
    const ChainScratch &c = s.chain;
    hipLaunchKernelGGL(pph_keys_kernel, dim3(grid), dim3(256), 0, stream, rec, n, a, c.keys0, c.idx0, s.sc);
    const hipError_t e = chain_sort_pairs(c, n, (int)a.key_bits, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(pph_walk_kernel, dim3(grid), dim3(256), 0, stream, rec, n, a, c.keys0, c.idx0, c.cnt, c.stage);
    return chain_scan_counts(c, n, &s.sc->steps, stream);
}

hipError_t pph_emit(const PphArgs &a, uint64_t n, const PphScratch &s, AdderSparseStep *d_steps, hipStream_t stream) {
    if (n == 0u) return hipSuccess;
    const hipError_t e = chain_scatter(s.chain, n, d_steps, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(pph_commit_kernel, dim3(grid_of(n)), dim3(256), 0, stream, n, a, s.chain.keys0);
    return hipGetLastError();
}

hipError_t pph_end_steps(const PphArgs &a, uint32_t running_t, AdderSparseStep *d_steps, PphScalars *sc,
                         hipStream_t stream) {
    hipLaunchKernelGGL(pph_init_scalars_kernel, dim3(1), dim3(1), 0, stream, sc);
    hipLaunchKernelGGL(pph_end_kernel, dim3(grid_of(a.units)), dim3(256), 0, stream, a, running_t, d_steps, sc);
    return hipGetLastError();
}

hipError_t pph_init_state(const PphArgs &a, hipStream_t stream) {
    hipLaunchKernelGGL(pph_init_state_kernel, dim3(grid_of(a.units)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t pph_times(const uint8_t *rec, uint64_t n, uint32_t *t, hipStream_t stream) {
    if (n == 0u) return hipSuccess;
    hipLaunchKernelGGL(pph_times_kernel, dim3(grid_of(n)), dim3(256), 0, stream, rec, n, t);
    return hipGetLastError();
}

hipError_t pph_exp_run(const double *x, double *y, uint64_t n, hipStream_t stream) {
    if (n == 0u) return hipSuccess;
    hipLaunchKernelGGL(pph_exp_kernel, dim3(grid_of(n)), dim3(256), 0, stream, x, y, n);
    return hipGetLastError();
}

}  // namespace adder
