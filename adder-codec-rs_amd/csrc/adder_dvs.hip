// adder_dvs.hip -- ADDER -> DVS conversion kernels (include/adder_dvs.h; adder-to-dvs/src/main.rs:241-363).
//
// The shape of adder_sparse.hip: units turn up anywhere in a batch and a unit's events form a serial chain.
//   1. keys: unit index per event (decoded from AdderEvents or 9 / 11-byte wire records), bad and EOF records
//      noted with atomicMin; a stable radix sort on ceil(log2(units + 1)) bits brings a unit's events together;
//   2. ln: a thread per SORTED event evaluates its log intensity.  In DeltaT it depends on the event alone; in
//      AbsoluteT on the event and its predecessor in the run (t' = t - the predecessor's time), both at hand here;
//      the first event of a unit with no state and d > 128 is bad;
//   3. walk: a thread per run chains the unit's integer time and the four-way test -- no transcendental on the
//      chain -- and marks the fired events (polarity, time) at their INPUT index;
//   4. an exclusive scan of the marks in input order places the DVS events, a thread per event stores them;
//   5. commit: the walked units' state is copied back unless the output did not fit.
// Everything past the first bad event (or EOF record) is left out of steps 3-5.
// A context that enabled the event video takes the VIDEO arm of steps 3 and 5 and the kernels of adder_dvs_video.hip
// between them; any other context launches exactly the steps above.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include "../../include/adder_dvs.h"
#include "adder_dvs_kernels.h"
#include "adder_log1p.hpp"
#include "adder_wire.hpp"

namespace adder {

__global__ void dvs_init_kernel(DvsScalars *sc, uint64_t n) {
    sc->bad = ~0ull;
    sc->eof = n;
    sc->total = 0ull;
}

template <int SRC>
__global__ __launch_bounds__(256) void dvs_keys_kernel(const void *__restrict__ in, uint64_t n, DvsArgs a,
                                                       uint32_t *__restrict__ keys, uint32_t *__restrict__ idx,
                                                       DvsScalars *sc) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const WireEv e = wire_load<SRC>(in, i);
    uint32_t key = a.units;  // sorted behind every unit, never walked
    if (e.end) {
        atomicMin(&sc->eof, (unsigned long long)i);
    } else {
        const bool in_plane = e.x < a.width && e.y < a.height && e.c < a.channels;
        if (!in_plane || (e.d > 128u && e.d < 255u)) atomicMin(&sc->bad, (unsigned long long)i);
        if (in_plane) key = (e.y * a.width + e.x) * a.channels + e.c;
    }
    keys[i] = key;
    idx[i] = (uint32_t)i;
}

template <int SRC>
__global__ __launch_bounds__(256) void dvs_ln_kernel(const void *__restrict__ in, uint64_t n, DvsArgs a,
                                                     const uint32_t *__restrict__ keys, const uint32_t *__restrict__ idx,
                                                     double *__restrict__ s_ln, uint64_t *__restrict__ s_td,
                                                     DvsScalars *sc) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j >= n) return;
    const uint32_t u = keys[j];
    if (u >= a.units) return;
    const uint32_t i = idx[j];
    const WireEv e = wire_load<SRC>(in, i);
    const bool head = j == 0u || keys[j - 1] != u;
    const bool init0 = a.cur_init[u] != 0u;
    const bool first = head && !init0;  // the unit's first event ever (main.rs:251-265)
    if (first && e.d > 128u) atomicMin(&sc->bad, (unsigned long long)i);
    uint32_t t = e.t;
    if (!first && !a.delta_t) {
        // AbsoluteT: event.t.saturating_sub(old_t as u32) (main.rs:272-273), old_t = the unit's time before it
        uint64_t old_t;
        if (head) {
            old_t = a.cur_t[u];
        } else {
            const uint32_t pt = wire_load<SRC>(in, idx[j - 1]).t;
            const bool prev_first = !init0 && (j - 1u == 0u || keys[j - 2] != u);
            old_t = (a.framed && !prev_first) ? wire_round_up(pt, a.ref) : (uint64_t)pt;
        }
        const uint32_t o = (uint32_t)old_t;
        t = t > o ? t - o : 0u;
    }
    s_ln[j] = e.d <= 128u ? dvs_intensity_ln(e.d, t, a.ref_f) : 0.0;
    s_td[j] = (uint64_t)e.t | ((uint64_t)e.d << 32);
}

// VIDEO: the arm of a context with the event video enabled -- every walked event also leaves the unit's time after
// it at its input index (0 for a unit's first event) and is counted for the count map.
template <bool VIDEO>
__global__ __launch_bounds__(256) void dvs_walk_kernel(uint64_t n, DvsArgs a, const uint32_t *__restrict__ keys,
                                                       const uint32_t *__restrict__ idx, const double *__restrict__ s_ln,
                                                       const uint64_t *__restrict__ s_td, uint8_t *__restrict__ flag,
                                                       uint64_t *__restrict__ tout, const DvsScalars *sc,
                                                       uint64_t *__restrict__ v_pt, const uint32_t *__restrict__ v_cur_cnt,
                                                       uint32_t *__restrict__ v_nxt_cnt) {
    const uint64_t j0 = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j0 >= n) return;
    const uint32_t u = keys[j0];
    if (u >= a.units || (j0 > 0u && keys[j0 - 1] == u)) return;  // a thread per run of one unit
    const uint64_t lim = wire_limit(sc->bad, sc->eof);
    bool init = a.cur_init[u] != 0u;
    double ln = a.cur_ln[u];
    uint64_t pt = a.cur_t[u];
    uint32_t walked = 0u;
    for (uint64_t j = j0; j < n && keys[j] == u; ++j) {
        const uint32_t i = idx[j];
        if (i >= lim) break;
        if (VIDEO) ++walked;
        const uint64_t td = s_td[j];
        const uint32_t d = (uint32_t)(td >> 32), t = (uint32_t)td;
        if (!init) {  // d <= 128 here: a first event with d > 128 set lim at or before it
            init = true;
            ln = s_ln[j];
            pt = t;
            continue;
        }
        const uint64_t old_t = pt;
        pt = a.delta_t ? pt + t : (uint64_t)t;
        if (a.framed) pt = wire_round_up(pt, a.ref);
        if (VIDEO) v_pt[i] = pt;
        if (d == 255u) continue;  // D_EMPTY: the time moved, nothing fires
        const double nw = s_ln[j];
        const bool win = nw > 0.406 && nw < 0.407;
        int p = -1;
        if (win && (ln > a.win_hi || (pt == old_t && ln > 0.6)))
            p = 1;
        else if (win && (ln < a.win_lo || (pt == old_t && ln < 0.3)))
            p = 0;
        else if (nw > ln + a.half)
            p = 1;
        else if (nw < ln - a.half)
            p = 0;
        if (p >= 0) {
            flag[i] = (uint8_t)(p + 1);
            tout[i] = old_t + 1u;
            ln = nw;
        }
    }
    a.nxt_init[u] = init ? 1u : 0u;
    a.nxt_ln[u] = ln;
    a.nxt_t[u] = pt;
    if (VIDEO) v_nxt_cnt[u] = v_cur_cnt[u] + walked;
}

struct DvsFired {
    __host__ __device__ __forceinline__ uint32_t operator()(uint8_t f) const { return f != 0u ? 1u : 0u; }
};

template <int SRC>
__global__ __launch_bounds__(256) void dvs_scatter_kernel(const void *__restrict__ in, uint64_t n,
                                                          const uint8_t *__restrict__ flag,
                                                          const uint64_t *__restrict__ tout,
                                                          const uint32_t *__restrict__ offs, int out_format,
                                                          void *__restrict__ out, uint64_t out_cap, DvsScalars *sc) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t f = flag[i];
    const uint64_t o = offs[i];
    if (i == n - 1u) sc->total = o + (f != 0u ? 1u : 0u);
    if (f == 0u || o >= out_cap) return;
    const WireEv e = wire_load<SRC>(in, i);
    const uint32_t p = f - 1u;
    if (out_format == ADDER_DVS_OUT_DAT) {
        uint2 r;
        r.x = (uint32_t)tout[i];
        r.y = (p << 28) | (e.y << 14) | e.x;  // x unmasked (main.rs:539-546)
        ((uint2 *)out)[o] = r;
    } else {
        AdderDvsEvent r;
        r.t = tout[i];
        r.x = (uint16_t)e.x;
        r.y = (uint16_t)e.y;
        r.p = (uint8_t)p;
        r.pad[0] = r.pad[1] = r.pad[2] = 0u;
        ((AdderDvsEvent *)out)[o] = r;
    }
}

// VIDEO: the video arm's verdict (the output and the frame ring both fit) decides, and the counts are committed too
template <bool VIDEO>
__global__ __launch_bounds__(256) void dvs_commit_kernel(uint64_t n, DvsArgs a, const uint32_t *__restrict__ keys,
                                                         uint64_t out_cap, const DvsScalars *sc,
                                                         const DvsVideoScalars *vs, uint32_t *__restrict__ v_cur_cnt,
                                                         const uint32_t *__restrict__ v_nxt_cnt) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j >= n) return;
    if (VIDEO ? vs->ok == 0ull : sc->total > out_cap) return;
    const uint32_t u = keys[j];
    if (u >= a.units || (j > 0u && keys[j - 1] == u)) return;
    a.cur_init[u] = a.nxt_init[u];
    a.cur_ln[u] = a.nxt_ln[u];
    a.cur_t[u] = a.nxt_t[u];
    if (VIDEO) v_cur_cnt[u] = v_nxt_cnt[u];
}

__global__ __launch_bounds__(256) void dvs_sort_keys_kernel(const void *__restrict__ rec, uint64_t n, int out_format,
                                                            uint32_t *__restrict__ keys, uint32_t *__restrict__ vals) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    keys[i] = out_format == ADDER_DVS_OUT_DAT ? ((const uint2 *)rec)[i].x
                                              : (uint32_t)((const AdderDvsEvent *)rec)[i].t;
    vals[i] = (uint32_t)i;
}

__global__ __launch_bounds__(256) void dvs_sort_gather_kernel(const void *__restrict__ rec, uint64_t n, int out_format,
                                                              const uint32_t *__restrict__ vals, void *__restrict__ tmp) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    if (out_format == ADDER_DVS_OUT_DAT)
        ((uint2 *)tmp)[i] = ((const uint2 *)rec)[vals[i]];
    else
        ((AdderDvsEvent *)tmp)[i] = ((const AdderDvsEvent *)rec)[vals[i]];
}

__global__ __launch_bounds__(256) void dvs_log1p_kernel(const double *__restrict__ x, double *__restrict__ y,
                                                        uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i < n) y[i] = dvs_log1p(x[i]);
}

size_t dvs_temp_bytes(uint64_t n) {
    size_t a = 0, b = 0;
    hipcub::DoubleBuffer<uint32_t> k(nullptr, nullptr), v(nullptr, nullptr);
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, a, k, v, (int)n);
    hipcub::TransformInputIterator<uint32_t, DvsFired, const uint8_t *> it(nullptr, DvsFired());
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, b, it, (uint32_t *)nullptr, (int)n);
    return (a > b ? a : b) + 256;
}

template <int SRC>
static hipError_t dvs_convert_src(const DvsArgs &a, const void *in, uint64_t n, int out_format, void *out,
                                  uint64_t out_cap, const DvsScratch &s, hipStream_t stream, const DvsVideoArgs *va) {
    const uint32_t grid = (uint32_t)((n + 255u) / 256u);
    size_t temp_bytes = s.temp_bytes;
    hipLaunchKernelGGL(dvs_init_kernel, dim3(1), dim3(1), 0, stream, s.sc, n);
    hipError_t e = hipMemsetAsync(s.flag, 0, n, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((dvs_keys_kernel<SRC>), dim3(grid), dim3(256), 0, stream, in, n, a, s.keys0, s.idx0, s.sc);
    hipcub::DoubleBuffer<uint32_t> k(s.keys0, s.keys1), v(s.idx0, s.idx1);
    e = hipcub::DeviceRadixSort::SortPairs(s.temp, temp_bytes, k, v, (int)n, 0, (int)a.key_bits, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((dvs_ln_kernel<SRC>), dim3(grid), dim3(256), 0, stream, in, n, a, k.Current(), v.Current(),
                       s.s_ln, s.s_td, s.sc);
    if (va) {
        e = hipMemsetAsync(va->pt, 0, n * 8u, stream);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(dvs_walk_kernel<true>, dim3(grid), dim3(256), 0, stream, n, a, k.Current(), v.Current(),
                           s.s_ln, s.s_td, s.flag, s.tout, s.sc, va->pt, va->cur_cnt, va->nxt_cnt);
    } else {
        hipLaunchKernelGGL(dvs_walk_kernel<false>, dim3(grid), dim3(256), 0, stream, n, a, k.Current(), v.Current(),
                           s.s_ln, s.s_td, s.flag, s.tout, s.sc, nullptr, nullptr, nullptr);
    }
    hipcub::TransformInputIterator<uint32_t, DvsFired, const uint8_t *> fired(s.flag, DvsFired());
    e = hipcub::DeviceScan::ExclusiveSum(s.temp, temp_bytes, fired, s.offs, (int)n, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((dvs_scatter_kernel<SRC>), dim3(grid), dim3(256), 0, stream, in, n, s.flag, s.tout, s.offs,
                       out_format, out, out_cap, s.sc);
    if (va) {
        e = dvs_video_schedule(a, *va, n, out_cap, s, stream);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(dvs_commit_kernel<true>, dim3(grid), dim3(256), 0, stream, n, a, k.Current(), out_cap, s.sc,
                           va->vs, va->cur_cnt, va->nxt_cnt);
        return va->draw ? dvs_video_draw(a, *va, SRC, in, n, s, stream) : hipGetLastError();
    }
    hipLaunchKernelGGL(dvs_commit_kernel<false>, dim3(grid), dim3(256), 0, stream, n, a, k.Current(), out_cap, s.sc,
                       nullptr, nullptr, nullptr);
    return hipGetLastError();
}

hipError_t dvs_convert(const DvsArgs &a, int source, const void *in, uint64_t n, int out_format, void *out,
                       uint64_t out_cap, const DvsScratch &s, hipStream_t stream, const DvsVideoArgs *va) {
    if (n == 0u) return hipSuccess;
    if (source == kSrcEvents) return dvs_convert_src<kSrcEvents>(a, in, n, out_format, out, out_cap, s, stream, va);
    if (source == kSrcWire9) return dvs_convert_src<kSrcWire9>(a, in, n, out_format, out, out_cap, s, stream, va);
    return dvs_convert_src<kSrcWire11>(a, in, n, out_format, out, out_cap, s, stream, va);
}

size_t dvs_sort_temp_bytes(uint64_t n) {
    size_t a = 0;
    hipcub::DoubleBuffer<uint32_t> k(nullptr, nullptr), v(nullptr, nullptr);
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, a, k, v, (int)n);
    return a + 256;
}

hipError_t dvs_sort(void *rec, uint64_t n, int out_format, uint32_t *keys0, uint32_t *keys1, uint32_t *vals0,
                    uint32_t *vals1, void *tmp, void *temp, size_t temp_bytes, hipStream_t stream) {
    if (n < 2u) return hipSuccess;
    const uint32_t grid = (uint32_t)((n + 255u) / 256u);
    hipLaunchKernelGGL(dvs_sort_keys_kernel, dim3(grid), dim3(256), 0, stream, rec, n, out_format, keys0, vals0);
    hipcub::DoubleBuffer<uint32_t> k(keys0, keys1), v(vals0, vals1);
    hipError_t e = hipcub::DeviceRadixSort::SortPairs(temp, temp_bytes, k, v, (int)n, 0, 32, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(dvs_sort_gather_kernel, dim3(grid), dim3(256), 0, stream, rec, n, out_format, v.Current(), tmp);
    const size_t rb = out_format == ADDER_DVS_OUT_DAT ? 8u : sizeof(AdderDvsEvent);
    e = hipMemcpyAsync(rec, tmp, n * rb, hipMemcpyDeviceToDevice, stream);
    if (e != hipSuccess) return e;
    return hipGetLastError();
}

hipError_t dvs_log1p_run(const double *x, double *y, uint64_t n, hipStream_t stream) {
    if (n == 0u) return hipSuccess;
    hipLaunchKernelGGL(dvs_log1p_kernel, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, stream, x, y, n);
    return hipGetLastError();
}

}  // namespace adder
