// adder_dvs_video.hip -- the DVS event video and the event-count map of adder-to-dvs (include/adder_dvs.h;
// adder-to-dvs/src/main.rs:195-239, 288, 382-411, 424-448) behind the conversion of adder_dvs.hip.  The arithmetic and
// its proof are in adder_dvs_video_logic.hpp; every step here is a thread per event or a device-wide scan, no
// workgroup waits for another.
//   1. the walk's video arm left pt[i], the unit's time after event i; its inclusive maximum gives current_t at every
//      position;
//   2. term: the stop value T_i of every position as max(T_i, F_0) - i; one inclusive minimum gives frame_count F_i;
//   3. reach: a fired event of frame g = (old_t + 1) / L is drawn iff g >= F_{i+1}; accept ? g + 1 : 0, whose inclusive
//      maximum is E at every position;
//   4. mark: position i emits frame F_i iff it pops and E_i > F_i; a scan places the emitted indices in `list`, the
//      last applied position leaves the state after the call and the verdict: the DVS output fits and the frames
//      [lo, E) fit the ring;
//   5. draw (after the commit, only on a good verdict): a stable sort of the accepted events by (frame, pixel) keeps
//      the last event in stream order of every run; it writes 255 / 0 into the ring;
//   6. hand-out (at pop time): the emitted frames are copied densely to the caller and their slots refilled with 128.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include "../../include/adder_dvs.h"
#include "adder_dvs_kernels.h"
#include "adder_dvs_video_logic.hpp"
#include "adder_wire.hpp"

namespace adder {

__global__ void dvsv_init_kernel(DvsVideoArgs va) {
    DvsVideoScalars *vs = va.vs;  // the values of a call that applies no event
    vs->F = va.F0;
    vs->E = va.E0;
    vs->cur = va.cur0;
    vs->n_emit = 0ull;
    vs->need = va.E0 > va.lo ? va.E0 - va.lo : 0ull;
    vs->ok = 1ull;
}

// current_t before event i: pt holds its inclusive maximum
__device__ __forceinline__ uint64_t dvsv_cur_before(const DvsVideoArgs &va, uint64_t i) {
    const uint64_t m = i == 0u ? 0u : va.pt[i - 1u];
    return va.cur0 > m ? va.cur0 : m;
}

__global__ __launch_bounds__(256) void dvsv_term_kernel(uint64_t n, DvsVideoArgs va) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    // positions past the call's limit are never read: any term does
    va.term[i] = dvs_video_term(dvs_video_stop(dvsv_cur_before(va, i), va.L, va.B), va.F0, i);
}

struct DvsvPos {
    uint64_t f;  // frame_count before the check
    bool pop;
};

// term holds its inclusive minimum
__device__ __forceinline__ DvsvPos dvsv_position(const DvsVideoArgs &va, uint64_t i) {
    DvsvPos p;
    p.f = dvs_video_frame_count(va.F0, i, i == 0u ? 0 : va.term[i - 1u]);
    p.pop = p.f < dvs_video_stop(dvsv_cur_before(va, i), va.L, va.B);
    return p;
}

__device__ __forceinline__ uint64_t dvsv_reach(const DvsVideoArgs &va, uint64_t i, uint64_t lim, const uint8_t *flag,
                                               const uint64_t *tout) {
    if (i >= lim || flag[i] == 0u) return 0u;
    const DvsvPos p = dvsv_position(va, i);
    return dvs_video_reach(true, tout[i], va.L, p.f + (p.pop ? 1u : 0u), va.draw != 0u);
}

__global__ __launch_bounds__(256) void dvsv_reach_kernel(uint64_t n, DvsVideoArgs va, const uint8_t *__restrict__ flag,
                                                         const uint64_t *__restrict__ tout, const DvsScalars *sc) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    va.reach[i] = dvsv_reach(va, i, wire_limit(sc->bad, sc->eof), flag, tout);
}

// reach holds its inclusive maximum
__global__ __launch_bounds__(256) void dvsv_mark_kernel(uint64_t n, DvsVideoArgs va, const DvsScalars *sc) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    uint8_t m = 0u;
    if (i < wire_limit(sc->bad, sc->eof)) {
        const DvsvPos p = dvsv_position(va, i);
        const uint64_t r = i == 0u ? 0u : va.reach[i - 1u];
        const uint64_t e = va.E0 > r ? va.E0 : r;
        m = p.pop && e > p.f ? 1u : 0u;
    }
    va.mark[i] = m;
}

struct DvsvMarked {
    __host__ __device__ __forceinline__ uint32_t operator()(uint8_t m) const { return m; }
};
struct DvsvMax {
    __host__ __device__ __forceinline__ uint64_t operator()(uint64_t a, uint64_t b) const { return a > b ? a : b; }
};
struct DvsvMin {
    __host__ __device__ __forceinline__ int64_t operator()(int64_t a, int64_t b) const { return a < b ? a : b; }
};

__global__ __launch_bounds__(256) void dvsv_list_kernel(uint64_t n, DvsVideoArgs va, uint64_t out_cap,
                                                        const DvsScalars *sc) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint64_t lim = wire_limit(sc->bad, sc->eof);
    if (i >= n || i >= lim) return;
    const DvsvPos p = dvsv_position(va, i);
    if (va.mark[i]) va.list[va.moffs[i]] = p.f;
    if (i != lim - 1u) return;
    // the last applied event: the state after the call and its verdict
    DvsVideoScalars *vs = va.vs;
    const uint64_t e = va.E0 > va.reach[i] ? va.E0 : va.reach[i];
    vs->F = p.f + (p.pop ? 1u : 0u);
    vs->E = e;
    vs->cur = va.cur0 > va.pt[i] ? va.cur0 : va.pt[i];
    vs->n_emit = (uint64_t)va.moffs[i] + va.mark[i];
    const uint64_t need = e > va.lo ? e - va.lo : 0u;
    vs->need = need;
    vs->ok = need <= va.ring_frames && sc->total <= out_cap ? 1ull : 0ull;
}

size_t dvs_video_temp_bytes(uint64_t n) {
    size_t a = 0, b = 0, c = 0, d = 0;
    hipcub::DoubleBuffer<uint64_t> k(nullptr, nullptr);
    hipcub::DoubleBuffer<uint32_t> v(nullptr, nullptr);
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, a, k, v, (int)n);
    (void)hipcub::DeviceScan::InclusiveScan(nullptr, b, (uint64_t *)nullptr, (uint64_t *)nullptr, DvsvMax(), (int)n);
    (void)hipcub::DeviceScan::InclusiveScan(nullptr, c, (int64_t *)nullptr, (int64_t *)nullptr, DvsvMin(), (int)n);
    hipcub::TransformInputIterator<uint32_t, DvsvMarked, const uint8_t *> it(nullptr, DvsvMarked());
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, d, it, (uint32_t *)nullptr, (int)n);
    size_t m = a > b ? a : b;
    m = m > c ? m : c;
    m = m > d ? m : d;
    return m + 256;
}

hipError_t dvs_video_schedule(const DvsArgs &a, const DvsVideoArgs &va, uint64_t n, uint64_t out_cap,
                              const DvsScratch &s, hipStream_t stream) {
    const uint32_t grid = (uint32_t)((n + 255u) / 256u);
    size_t tb = va.temp_bytes;
    hipLaunchKernelGGL(dvsv_init_kernel, dim3(1), dim3(1), 0, stream, va);
    hipError_t e = hipcub::DeviceScan::InclusiveScan(va.temp, tb, va.pt, va.pt, DvsvMax(), (int)n, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(dvsv_term_kernel, dim3(grid), dim3(256), 0, stream, n, va);
    e = hipcub::DeviceScan::InclusiveScan(va.temp, tb, va.term, va.term, DvsvMin(), (int)n, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(dvsv_reach_kernel, dim3(grid), dim3(256), 0, stream, n, va, s.flag, s.tout, s.sc);
    e = hipcub::DeviceScan::InclusiveScan(va.temp, tb, va.reach, va.reach, DvsvMax(), (int)n, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(dvsv_mark_kernel, dim3(grid), dim3(256), 0, stream, n, va, s.sc);
    hipcub::TransformInputIterator<uint32_t, DvsvMarked, const uint8_t *> marked(va.mark, DvsvMarked());
    e = hipcub::DeviceScan::ExclusiveSum(va.temp, tb, marked, va.moffs, (int)n, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(dvsv_list_kernel, dim3(grid), dim3(256), 0, stream, n, va, out_cap, s.sc);
    return hipGetLastError();
}

// ---- draw ----

// The key of event i: (its frame - lo) * w * h + y * w + x, or `none` (sorted behind every pixel) when it is not drawn.
// reach[i] (a running maximum by now) cannot say whether i was accepted, so the accept test is made again.
template <int SRC>
__global__ __launch_bounds__(256) void dvsv_keys_kernel(const void *__restrict__ in, uint64_t n, DvsArgs a,
                                                        DvsVideoArgs va, const uint8_t *__restrict__ flag,
                                                        const uint64_t *__restrict__ tout, const DvsScalars *sc,
                                                        uint64_t none) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    uint64_t key = none;
    if (va.vs->ok != 0ull) {
        const uint64_t r = dvsv_reach(va, i, wire_limit(sc->bad, sc->eof), flag, tout);
        if (r != 0u) {  // frame r - 1 in [lo, lo + ring_frames): the verdict bounds E - lo
            const WireEv e = wire_load<SRC>(in, i);
            key = (r - 1u - va.lo) * ((uint64_t)a.width * a.height) + (uint64_t)e.y * a.width + e.x;
        }
    }
    va.k0[i] = key;
    va.v0[i] = (uint32_t)i;
}

__global__ __launch_bounds__(256) void dvsv_draw_kernel(uint64_t n, DvsArgs a, DvsVideoArgs va,
                                                        const uint64_t *__restrict__ keys,
                                                        const uint32_t *__restrict__ vals,
                                                        const uint8_t *__restrict__ flag, uint64_t none) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j >= n) return;
    const uint64_t key = keys[j];
    if (key >= none || (j + 1u < n && keys[j + 1u] == key)) return;  // the last of its run: the latest in the stream
    const uint64_t wh = (uint64_t)a.width * a.height;
    const uint64_t slot = (va.lo + key / wh) % va.ring_frames;
    va.ring[slot * wh + key % wh] = flag[vals[j]] == 2u ? (uint8_t)255 : (uint8_t)0;
}

template <int SRC>
static hipError_t dvsv_draw_src(const DvsArgs &a, const DvsVideoArgs &va, const void *in, uint64_t n,
                                const DvsScratch &s, hipStream_t stream) {
    const uint32_t grid = (uint32_t)((n + 255u) / 256u);
    const uint64_t none = va.ring_frames * (uint64_t)a.width * a.height;
    hipLaunchKernelGGL((dvsv_keys_kernel<SRC>), dim3(grid), dim3(256), 0, stream, in, n, a, va, s.flag, s.tout, s.sc,
                       none);
    hipcub::DoubleBuffer<uint64_t> k(va.k0, va.k1);
    hipcub::DoubleBuffer<uint32_t> v(va.v0, va.v1);
    size_t tb = va.temp_bytes;
    uint32_t bits = 1;
    while (bits < 64u && (1ull << bits) < none + 1u) ++bits;
    const hipError_t e = hipcub::DeviceRadixSort::SortPairs(va.temp, tb, k, v, (int)n, 0, (int)bits, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(dvsv_draw_kernel, dim3(grid), dim3(256), 0, stream, n, a, va, k.Current(), v.Current(), s.flag,
                       none);
    return hipGetLastError();
}

hipError_t dvs_video_draw(const DvsArgs &a, const DvsVideoArgs &va, int source, const void *in, uint64_t n,
                          const DvsScratch &s, hipStream_t stream) {
    if (source == kSrcEvents) return dvsv_draw_src<kSrcEvents>(a, va, in, n, s, stream);
    if (source == kSrcWire9) return dvsv_draw_src<kSrcWire9>(a, va, in, n, s, stream);
    return dvsv_draw_src<kSrcWire11>(a, va, in, n, s, stream);
}

// ---- hand-out ----

// T = uint4 when a plane is a whole number of 16-byte words and the caller's buffer is aligned (every ring slot then
// is as well), else uint8_t.  Adjacent lanes take adjacent words; a word is read, handed out and refilled by one lane.
template <typename T>
__global__ __launch_bounds__(256) void dvsv_handout_kernel(T *__restrict__ ring, uint64_t ring_frames,
                                                           uint64_t plane_words, const uint64_t *__restrict__ list,
                                                           uint64_t k, T *__restrict__ out, T blank) {
    const uint64_t total = k * plane_words;
    const uint64_t stride = (uint64_t)gridDim.x * 256u;
    for (uint64_t u = (uint64_t)blockIdx.x * 256u + threadIdx.x; u < total; u += stride) {
        const uint64_t q = u / plane_words;
        T *src = ring + (list[q] % ring_frames) * plane_words + (u - q * plane_words);
        out[u] = *src;
        *src = blank;
    }
}

constexpr uint32_t kHandoutMaxBlocks = 2048;  // 8 blocks per CU of 256: more only queue behind them

hipError_t dvs_video_handout(const DvsArgs &a, const DvsVideoArgs &va, const uint64_t *d_list, uint64_t k,
                             uint8_t *d_out, hipStream_t stream) {
    if (k == 0u) return hipSuccess;
    const uint64_t wh = (uint64_t)a.width * a.height;
    const bool wide = wh % 16u == 0u && ((uintptr_t)d_out & 15u) == 0u;
    const uint64_t words = wide ? wh / 16u : wh;
    const uint64_t blocks = (k * words + 255u) / 256u;
    const uint32_t grid = (uint32_t)(blocks < kHandoutMaxBlocks ? blocks : kHandoutMaxBlocks);
    if (wide) {
        const uint4 blank = make_uint4(0x80808080u, 0x80808080u, 0x80808080u, 0x80808080u);
        hipLaunchKernelGGL(dvsv_handout_kernel<uint4>, dim3(grid), dim3(256), 0, stream, (uint4 *)va.ring,
                           va.ring_frames, words, d_list, k, (uint4 *)d_out, blank);
    } else {
        hipLaunchKernelGGL(dvsv_handout_kernel<uint8_t>, dim3(grid), dim3(256), 0, stream, va.ring, va.ring_frames,
                           words, d_list, k, d_out, (uint8_t)128);
    }
    return hipGetLastError();
}

// ---- count map ----

__global__ __launch_bounds__(256) void dvsv_count_peak_kernel(uint32_t units, const uint32_t *__restrict__ cnt,
                                                              uint32_t *m) {
    const uint32_t u = blockIdx.x * 256u + threadIdx.x;
    uint32_t v = u < units ? dvs_video_count_peak(cnt[u]) : 0u;
    for (int o = 32; o > 0; o >>= 1) {  // the wave's maximum, one atomic per wave
        const uint32_t w = __shfl_xor(v, o);
        v = v > w ? v : w;
    }
    if ((threadIdx.x & 63u) == 0u && v != 0u) atomicMax(m, v);
}

__global__ __launch_bounds__(256) void dvsv_count_fill_kernel(uint64_t pixels, uint32_t channels,
                                                              const uint32_t *__restrict__ cnt, const uint32_t *m,
                                                              uint8_t *__restrict__ out) {
    const uint64_t b = (uint64_t)blockIdx.x * 256u + threadIdx.x;  // a thread per output byte
    if (b >= pixels * 3u) return;
    const uint64_t px = b / 3u;
    const uint32_t c = (uint32_t)(b - px * 3u);
    out[b] = c < channels ? dvs_video_count_byte(cnt[px * channels + c], *m) : (uint8_t)128;
}

hipError_t dvs_video_count_map(const DvsArgs &a, const uint32_t *d_cnt, uint32_t *d_m, uint8_t *d_out,
                               hipStream_t stream) {
    hipError_t e = hipMemsetAsync(d_m, 0, 4u, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(dvsv_count_peak_kernel, dim3((a.units + 255u) / 256u), dim3(256), 0, stream, a.units, d_cnt, d_m);
    const uint64_t pixels = (uint64_t)a.width * a.height;
    hipLaunchKernelGGL(dvsv_count_fill_kernel, dim3((uint32_t)((pixels * 3u + 255u) / 256u)), dim3(256), 0, stream, pixels,
                       a.channels, d_cnt, d_m, d_out);
    return hipGetLastError();
}

}  // namespace adder
