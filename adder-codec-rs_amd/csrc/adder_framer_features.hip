// adder_framer_features.hip -- gfx950 kernels of feature detection while framing (FrameSequence::detect_features,
// framer/driver.rs:482-553; logic in adder_framer_features.hpp).
//
// The reference tests event i against one plane that holds every earlier event of the stream.  Here:
//   1. keys: unit index per event; a stable radix sort on ceil(log2(units + 1)) bits gives every unit its events in
//      input order (the shape of adder_dvs.hip);
//   2. walk: a thread per run applies framer_step to the unit's chain -- the framing itself, as
//      adder_framer_segment_kernel does it -- and leaves val8 (by sorted position and by input index), t_after
//      (by input index) and the run's bounds;
//   3. candidates: a thread per event in input order.  t[i] != t_after[i - 1], channel 0, off the border; then each
//      ring pixel's value is the val8 of the last event of that pixel's run with an index below i (binary search),
//      or the carried plane.  The four opposite pairs come first, most candidates stop there;
//   4. an exclusive scan of the marks in input order places the feature records, a thread per event stores them;
//   5. commit: the last event of every run writes the plane, the call's last t_after becomes the carried one.
// The plane is read by step 3 and written by step 5 only, so a ring pixel without an earlier event in the call reads
// what the previous call left.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include "adder_framer_features.h"

namespace adder {

__device__ __forceinline__ void feat_ring_store(uint8_t *ring, size_t idx, uint32_t value_type, uint32_t v) {
    if (value_type == 0u) ring[idx] = (uint8_t)v;
    else if (value_type == 1u) reinterpret_cast<uint16_t *>(ring)[idx] = (uint16_t)v;
    else reinterpret_cast<uint32_t *>(ring)[idx] = v;
}

__global__ __launch_bounds__(256) void framer_feat_keys_kernel(const uint32_t *__restrict__ ev, uint32_t n, FramerArgs a,
                                                               uint32_t *__restrict__ keys, uint32_t *__restrict__ idx,
                                                               uint8_t *__restrict__ val8_input,
                                                               uint32_t *__restrict__ t_after) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t xy = ev[3u * (size_t)i], cd = ev[3u * (size_t)i + 1u];
    const uint32_t x = xy & 0xffffu, y = xy >> 16;
    uint32_t c = cd & 0xffu;
    c = c == 0xffu ? 0u : c;  // coord.c.unwrap_or(0)
    uint32_t key = a.n_units;  // sorted behind every unit, never walked
    if (x < a.width && y >= a.row_begin && y - a.row_begin < a.rows && c < a.channels) {
        key = ((y - a.row_begin) * a.width + x) * a.channels + c;
    } else {
        atomicOr(a.status, kFramerStatusMalformed);
        val8_input[i] = 0u;
        t_after[i] = ev[3u * (size_t)i + 2u];
    }
    keys[i] = key;
    idx[i] = i;
}

__global__ __launch_bounds__(256) void framer_feat_walk_kernel(const uint32_t *__restrict__ ev, uint32_t n, FramerArgs a,
                                                               const uint32_t *__restrict__ keys,
                                                               const uint32_t *__restrict__ idx,
                                                               uint8_t *__restrict__ val8_sorted,
                                                               uint8_t *__restrict__ val8_input,
                                                               uint32_t *__restrict__ t_after, uint2 *__restrict__ runs) {
    const uint32_t j0 = blockIdx.x * 256u + threadIdx.x;
    if (j0 >= n) return;
    const uint32_t u = keys[j0];
    if (u >= a.n_units || (j0 > 0u && keys[j0 - 1u] == u)) return;  // a thread per run of one unit
    FramerPx p = a.px[u];
    uint32_t flags = 0u, j = j0;
    for (; j < n && keys[j] == u; ++j) {
        const uint32_t i = idx[j];
        const uint32_t cd = ev[3u * (size_t)i + 1u], t = ev[3u * (size_t)i + 2u];
        const FramerFeatureStep o = framer_feature_step(p, (cd >> 8) & 0xffu, t, a.k);
        if (o.overflow) flags |= kFramerStatusRange;
        if (o.fills) {
            // frames (from, to]; those already handed out (below frames_written) are skipped (driver.rs:1074-1075)
            int32_t f = o.from + 1 > a.frames_written ? o.from + 1 : a.frames_written;
            for (; f <= o.to; ++f) {
                if ((uint32_t)(f - a.frames_written) >= a.ring_frames) {
                    flags |= kFramerStatusRing;
                    break;
                }
                feat_ring_store(a.ring, (size_t)((uint32_t)f % a.ring_frames) * a.n_units + u, a.k.value_type, p.lasti);
            }
        }
        val8_sorted[j] = (uint8_t)o.val8;
        val8_input[i] = (uint8_t)o.val8;
        t_after[i] = o.t_after;
    }
    a.px[u] = p;
    runs[u] = make_uint2(j0, j);
    if (flags) atomicOr(a.status, flags);
}

__global__ __launch_bounds__(256) void framer_feat_candidates_kernel(
    const uint32_t *__restrict__ ev, uint32_t n, FramerArgs a, const uint32_t *__restrict__ idx,
    const uint8_t *__restrict__ val8_sorted, const uint8_t *__restrict__ val8_input,
    const uint32_t *__restrict__ t_after, const uint2 *__restrict__ runs, const uint8_t *__restrict__ plane,
    const uint32_t *__restrict__ carry, uint8_t *__restrict__ mark) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t xy = ev[3u * (size_t)i], cd = ev[3u * (size_t)i + 1u], t = ev[3u * (size_t)i + 2u];
    const uint32_t x = xy & 0xffffu, y = xy >> 16;
    const bool last_valid = i > 0u ? true : carry[0] != 0u;
    const uint32_t last_t = i > 0u ? t_after[i - 1u] : carry[1];
    bool feature = false;
    // (full plane only: a.rows = height, a.row_begin = 0)
    if (framer_feature_is_candidate(x, y, cd & 0xffu, t, last_valid, last_t, a.width, a.rows)) {
        const int centre = (int)val8_input[i];
        feature = fast9_ring_is_feature(centre, [&](uint32_t k) -> int {
            const uint32_t rx = (uint32_t)((int)x + fast_ring_dx(k)), ry = (uint32_t)((int)y + fast_ring_dy(k));
            const uint32_t ru = (ry * a.width + rx) * a.channels;  // channel 0 of the ring pixel (cv.rs:77-87)
            const uint2 r = runs[ru];
            return (int)framer_feature_value_before(idx, val8_sorted, r.x, r.y, i, plane[ru]);
        });
    }
    mark[i] = feature ? 1u : 0u;
}

struct FeatMarked {
    __host__ __device__ __forceinline__ uint32_t operator()(uint8_t f) const { return f != 0u ? 1u : 0u; }
};

__global__ __launch_bounds__(256) void framer_feat_scatter_kernel(const uint32_t *__restrict__ ev, uint32_t n,
                                                                  uint64_t index_base, const uint8_t *__restrict__ mark,
                                                                  const uint32_t *__restrict__ offs,
                                                                  AdderFramerFeature *__restrict__ out, uint64_t out_cap,
                                                                  uint32_t *__restrict__ count) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t f = mark[i], o = offs[i];
    if (i == n - 1u) *count = o + f;
    if (f == 0u || (uint64_t)o >= out_cap) return;
    const uint32_t xy = ev[3u * (size_t)i];
    AdderFramerFeature r;
    r.index = index_base + i;
    r.t = ev[3u * (size_t)i + 2u];  // the raw t, also in a DeltaT stream (driver.rs:446)
    r.x = (uint16_t)(xy & 0xffffu);
    r.y = (uint16_t)(xy >> 16);
    out[o] = r;
}

__global__ __launch_bounds__(256) void framer_feat_commit_kernel(uint32_t n, uint32_t n_units,
                                                                 const uint32_t *__restrict__ keys,
                                                                 const uint8_t *__restrict__ val8_sorted,
                                                                 const uint32_t *__restrict__ t_after,
                                                                 uint8_t *__restrict__ plane, uint32_t *__restrict__ carry) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n) return;
    if (j == 0u) {
        carry[0] = 1u;
        carry[1] = t_after[n - 1u];
    }
    const uint32_t u = keys[j];
    if (u >= n_units || (j + 1u < n && keys[j + 1u] == u)) return;  // the last event of a run
    plane[u] = val8_sorted[j];
}

size_t framer_features_temp_bytes(uint64_t n) {
    size_t a = 0, b = 0;
    hipcub::DoubleBuffer<uint32_t> k(nullptr, nullptr), v(nullptr, nullptr);
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, a, k, v, (int)n);
    hipcub::TransformInputIterator<uint32_t, FeatMarked, const uint8_t *> it(nullptr, FeatMarked());
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, b, it, (uint32_t *)nullptr, (int)n);
    return (a > b ? a : b) + 256;
}

hipError_t framer_features_run(const uint32_t *ev, uint64_t n64, uint64_t index_base, const FramerArgs &a,
                               uint32_t key_bits, const FramerFeatureScratch &s, const FramerFeatureState &st,
                               hipStream_t stream) {
    if (n64 == 0u) return hipSuccess;
    const uint32_t n = (uint32_t)n64;  // the caller keeps n below 2^31
    const uint32_t grid = (n + 255u) / 256u;
    size_t temp_bytes = s.temp_bytes;
    hipError_t e = hipMemsetAsync(s.runs, 0, (size_t)a.n_units * sizeof(uint2), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(framer_feat_keys_kernel, dim3(grid), dim3(256), 0, stream, ev, n, a, s.keys0, s.idx0,
                       s.val8_input, s.t_after);
    hipcub::DoubleBuffer<uint32_t> k(s.keys0, s.keys1), v(s.idx0, s.idx1);
    e = hipcub::DeviceRadixSort::SortPairs(s.temp, temp_bytes, k, v, (int)n, 0, (int)key_bits, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(framer_feat_walk_kernel, dim3(grid), dim3(256), 0, stream, ev, n, a, k.Current(), v.Current(),
                       s.val8_sorted, s.val8_input, s.t_after, s.runs);
    hipLaunchKernelGGL(framer_feat_candidates_kernel, dim3(grid), dim3(256), 0, stream, ev, n, a, v.Current(),
                       s.val8_sorted, s.val8_input, s.t_after, s.runs, st.plane, st.carry, s.mark);
    hipcub::TransformInputIterator<uint32_t, FeatMarked, const uint8_t *> marked(s.mark, FeatMarked());
    temp_bytes = s.temp_bytes;
    e = hipcub::DeviceScan::ExclusiveSum(s.temp, temp_bytes, marked, s.offs, (int)n, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(framer_feat_scatter_kernel, dim3(grid), dim3(256), 0, stream, ev, n, index_base, s.mark, s.offs,
                       st.out, st.out_cap, st.count);
    hipLaunchKernelGGL(framer_feat_commit_kernel, dim3(grid), dim3(256), 0, stream, n, a.n_units, k.Current(),
                       s.val8_sorted, s.t_after, st.plane, st.carry);
    return hipGetLastError();
}

}  // namespace adder
