// adder_player.hip -- the latest-event player's kernels (include/adder_player.h; adder_video_player.rs:52-216).
//
// The shape of adder_dvs.hip, with two pieces of its own (the display schedule and the frame hand-out):
//   1. keys: unit index per record (AdderEvents or 9 / 11-byte wire records); a record with d > 128 gets the key
//      `units` and takes part in nothing; events outside the plane and EOF records are noted with atomicMin; a stable
//      radix sort on ceil(log2(units + 1)) bits brings a unit's events together, input indices ascending in a run;
//   2. values: a thread per SORTED event.  AbsoluteT needs only the run predecessor (or the carried last_ts): value,
//      rounded last_ts and the candidate for current_t are all written here.  In the other modes last_ts is a chain:
//      the value is written here, a thread per run then walks the times (u32 adds and the round-up, nothing else);
//   3. clock: candidates sit in input order behind the carried current_t; an inclusive prefix maximum gives current_t
//      before every check;
//   4. schedule (adder_player_logic.hpp): term_i = max(T_i, F_0) - i, an inclusive prefix minimum, the marks
//      [F_i < T_i], an exclusive sum and a compaction to the display positions s_0 < s_1 < ...;
//   5. hand-out: a thread per (frame, unit) looks the unit's last event before s_k up in the unit's run;
//   6. commit: the last applied event of every run leaves display[u] and last_ts[u].
// The host waits once between 4 and 5 (the frame count sizes the hand-out's grid and decides whether 5 and 6 run).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include "../../include/adder_player.h"
#include "adder_player_kernels.h"
#include "adder_player_logic.hpp"
#include "adder_wire.hpp"

namespace adder {

__global__ void player_init_kernel(PlayerScalars *sc, uint64_t n, uint32_t *cand, uint32_t cur0) {
    sc->bad = ~0ull;
    sc->eof = n;
    sc->total = 0ull;
    sc->cur = cur0;
    cand[0] = cur0;
}

template <int SRC>
__global__ __launch_bounds__(256) void player_keys_kernel(const void *__restrict__ in, uint64_t n, PlayerArgs a,
                                                          uint32_t *__restrict__ keys, uint32_t *__restrict__ idx,
                                                          PlayerScalars *sc) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const WireEv e = wire_load<SRC>(in, i);
    uint32_t key = a.units;
    if (e.end) {
        atomicMin(&sc->eof, (unsigned long long)i);
    } else if (e.d <= 128u) {  // d > 128 never indexes the plane (adder_video_player.rs:134)
        if (e.x < a.width && e.y < a.height && e.c < a.channels)
            key = (e.y * a.width + e.x) * a.channels + e.c;
        else
            atomicMin(&sc->bad, (unsigned long long)i);
    }
    keys[i] = key;
    idx[i] = (uint32_t)i;
}

// Reads a record per thread, writes 12 B per event (value, time) and in AbsoluteT the 4 B candidate at its input index.
template <int SRC>
__global__ __launch_bounds__(256) void player_value_kernel(const void *__restrict__ in, uint64_t n, PlayerArgs a,
                                                           const uint32_t *__restrict__ keys,
                                                           const uint32_t *__restrict__ idx, double *__restrict__ s_val,
                                                           uint32_t *__restrict__ s_ts, uint32_t *__restrict__ cand,
                                                           const PlayerScalars *sc) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j >= n) return;
    const uint32_t u = keys[j];
    if (u >= a.units) return;
    const uint32_t i = idx[j];
    const WireEv e = wire_load<SRC>(in, i);
    if (!a.absolute) {
        s_val[j] = player_value(e.d, e.t, a.ref_f, a.m);
        s_ts[j] = e.t;  // the walk turns it into last_ts
        return;
    }
    const bool head = j == 0u || keys[j - 1] != u;
    const uint32_t prev = head ? a.last_ts[u] : player_round_up(wire_load<SRC>(in, idx[j - 1]).t, a.ref);
    s_val[j] = player_value(e.d, e.t - prev, a.ref_f, a.m);
    s_ts[j] = player_round_up(e.t, a.ref);
    if (i < wire_limit(sc->bad, sc->eof)) cand[(uint64_t)i + 1u] = e.t;
}

// A thread per run: last_ts += t, rounded up, in u32 (the reference's wrap-around exactly).
__global__ __launch_bounds__(256) void player_walk_kernel(uint64_t n, PlayerArgs a, const uint32_t *__restrict__ keys,
                                                          const uint32_t *__restrict__ idx, uint32_t *__restrict__ s_ts,
                                                          uint32_t *__restrict__ cand, const PlayerScalars *sc) {
    const uint64_t j0 = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j0 >= n) return;
    const uint32_t u = keys[j0];
    if (u >= a.units || (j0 > 0u && keys[j0 - 1] == u)) return;
    const uint64_t lim = wire_limit(sc->bad, sc->eof);
    uint32_t ts = a.last_ts[u];
    for (uint64_t j = j0; j < n && keys[j] == u; ++j) {
        const uint32_t i = idx[j];
        if (i >= lim) break;
        ts = player_round_up(ts + s_ts[j], a.ref);
        s_ts[j] = ts;
        cand[(uint64_t)i + 1u] = ts;
    }
}

__global__ __launch_bounds__(256) void player_term_kernel(uint64_t m, PlayerArgs a, uint64_t f0,
                                                          const uint32_t *__restrict__ cur, int64_t *__restrict__ term) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i < m) term[i] = player_term(player_stop(cur[i], a.fl), f0, i);
}

__global__ __launch_bounds__(256) void player_mark_kernel(uint64_t n, int final_check, PlayerArgs a, uint64_t f0,
                                                          const uint32_t *__restrict__ cur,
                                                          const int64_t *__restrict__ pmin, uint8_t *__restrict__ mark,
                                                          PlayerScalars *sc) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i > n) return;
    const uint64_t lim = wire_limit(sc->bad, sc->eof);
    // checks: one before every applied event; one more where the stream ends (EOF record) or the caller says so
    const bool last = sc->bad < sc->eof ? false : (sc->eof < n || final_check != 0);
    const uint64_t nchk = lim + (last ? 1u : 0u);
    if (i == lim) sc->cur = cur[i];
    const uint64_t f = player_frame_count(f0, i, i > 0u ? pmin[i - 1] : 0);
    mark[i] = (i < nchk && f < player_stop(cur[i], a.fl)) ? 1u : 0u;
}

struct PlayerMarked {
    __host__ __device__ __forceinline__ uint32_t operator()(uint8_t f) const { return f; }
};

__global__ __launch_bounds__(256) void player_compact_kernel(uint64_t n, const uint8_t *__restrict__ mark,
                                                             const uint32_t *__restrict__ offs,
                                                             uint32_t *__restrict__ pos, PlayerScalars *sc) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i > n) return;
    if (mark[i]) pos[offs[i]] = (uint32_t)i;
    if (i == n) sc->total = (unsigned long long)offs[i] + mark[i];
}

// run_lo[u] = the first sorted position whose key is >= u, for u in 0..=units (units + 1 threads)
__global__ __launch_bounds__(256) void player_bounds_kernel(uint64_t n, PlayerArgs a, const uint32_t *__restrict__ keys) {
    const uint32_t u = blockIdx.x * 256u + threadIdx.x;
    if (u > a.units) return;
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (keys[mid] < u)
            lo = mid + 1u;
        else
            hi = mid;
    }
    a.run_lo[u] = (uint32_t)lo;
}

// The value unit u shows at display position s: its last event with input index < s, else the carried matrix.
__device__ __forceinline__ double player_lookup(const PlayerArgs &a, uint32_t u, uint32_t s,
                                                const uint32_t *__restrict__ idx, const double *__restrict__ s_val) {
    uint32_t lo = a.run_lo[u];
    const uint32_t first = lo;
    uint32_t hi = a.run_lo[u + 1u];
    while (lo < hi) {  // idx ascends within a run (stable sort): count the entries below s
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (idx[mid] < s)
            lo = mid + 1u;
        else
            hi = mid;
    }
    return lo > first ? s_val[lo - 1u] : a.display[u];
}

// The hot path.  The frames are one flat array of n_frames * units elements; a thread owns PER adjacent elements
// (1 f64 = 8 B, or 4 u8 = one dword), adjacent threads adjacent elements: every store instruction of a wave covers
// 512 B (f64) or 256 B (u8) of consecutive memory.  Bytes moved: WRITES n_frames * units * sizeof(OUT), each byte once;
// READS per element 8 B of run bounds (shared by the frames of a unit, cached), ceil(log2(run + 1)) 4-B probes of the
// unit's run and one 8-B value (s_val or display).  At 1080p one f64 frame is 16.6 MB written against a batch's events.
template <typename OUT, int PER>
__global__ __launch_bounds__(256) void player_handout_kernel(PlayerArgs a, uint64_t total,
                                                             const uint32_t *__restrict__ idx,
                                                             const double *__restrict__ s_val,
                                                             const uint32_t *__restrict__ pos, OUT *__restrict__ out) {
    const uint64_t g = ((uint64_t)blockIdx.x * 256u + threadIdx.x) * (uint64_t)PER;
    if (g >= total) return;
    uint64_t k = g / a.units;
    uint32_t u = (uint32_t)(g - k * a.units);
    if (PER == 1) {
        const double v = player_lookup(a, u, pos[k], idx, s_val);
        if (sizeof(OUT) == 8u)
            ((double *)out)[g] = v;
        else
            ((uint8_t *)out)[g] = player_to_u8(v);
        return;
    }
    uint32_t s = pos[k];
    uint32_t packed = 0u;
    const uint32_t cnt = total - g < (uint64_t)PER ? (uint32_t)(total - g) : (uint32_t)PER;
    for (uint32_t e = 0; e < cnt; ++e) {
        packed |= (uint32_t)player_to_u8(player_lookup(a, u, s, idx, s_val)) << (8u * e);
        if (++u == a.units && e + 1u < cnt) {  // the next element opens the next frame
            u = 0u;
            s = pos[++k];
        }
    }
    if (cnt == (uint32_t)PER) {
        *(uint32_t *)((uint8_t *)out + g) = packed;  // g is a multiple of 4, the buffer 8-byte aligned
    } else {
        for (uint32_t e = 0; e < cnt; ++e) ((uint8_t *)out)[g + e] = (uint8_t)(packed >> (8u * e));
    }
}

__global__ __launch_bounds__(256) void player_commit_kernel(uint64_t n, uint64_t lim, PlayerArgs a,
                                                            const uint32_t *__restrict__ keys,
                                                            const uint32_t *__restrict__ idx,
                                                            const double *__restrict__ s_val,
                                                            const uint32_t *__restrict__ s_ts) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j >= n) return;
    const uint32_t u = keys[j];
    if (u >= a.units || idx[j] >= lim) return;
    if (j + 1u < n && keys[j + 1] == u && idx[j + 1] < lim) return;  // not the unit's last applied event
    a.display[u] = s_val[j];
    a.last_ts[u] = s_ts[j];
}

__global__ __launch_bounds__(256) void player_display_kernel(PlayerArgs a, uint8_t *__restrict__ out) {
    const uint32_t u = blockIdx.x * 256u + threadIdx.x;
    if (u < a.units) out[u] = player_to_u8(a.display[u]);
}

size_t player_temp_bytes(uint64_t n) {
    size_t a = 0, b = 0, c = 0, d = 0;
    const int m = (int)(n + 1u);
    hipcub::DoubleBuffer<uint32_t> k(nullptr, nullptr), v(nullptr, nullptr);
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, a, k, v, (int)n);
    (void)hipcub::DeviceScan::InclusiveScan(nullptr, b, (const uint32_t *)nullptr, (uint32_t *)nullptr, hipcub::Max(), m);
    (void)hipcub::DeviceScan::InclusiveScan(nullptr, c, (const int64_t *)nullptr, (int64_t *)nullptr, hipcub::Min(), m);
    hipcub::TransformInputIterator<uint32_t, PlayerMarked, const uint8_t *> it(nullptr, PlayerMarked());
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, d, it, (uint32_t *)nullptr, m);
    if (b > a) a = b;
    if (c > a) a = c;
    if (d > a) a = d;
    return a + 256;
}

template <int SRC>
static hipError_t player_schedule_src(const PlayerArgs &a, const void *in, uint64_t n, int final_check, uint32_t cur0,
                                      uint64_t f0, PlayerScratch &s, hipStream_t stream) {
    const uint64_t m = n + 1u;
    const uint32_t grid = (uint32_t)((n + 255u) / 256u), grid_m = (uint32_t)((m + 255u) / 256u);
    size_t temp_bytes = s.temp_bytes;
    hipError_t e = hipMemsetAsync(s.cand, 0, m * 4u, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(player_init_kernel, dim3(1), dim3(1), 0, stream, s.sc, n, s.cand, cur0);
    s.keys = s.keys0;
    s.idx = s.idx0;
    if (n > 0u) {
        hipLaunchKernelGGL((player_keys_kernel<SRC>), dim3(grid), dim3(256), 0, stream, in, n, a, s.keys0, s.idx0, s.sc);
        hipcub::DoubleBuffer<uint32_t> k(s.keys0, s.keys1), v(s.idx0, s.idx1);
        e = hipcub::DeviceRadixSort::SortPairs(s.temp, temp_bytes, k, v, (int)n, 0, (int)a.key_bits, stream);
        if (e != hipSuccess) return e;
        s.keys = k.Current();
        s.idx = v.Current();
        hipLaunchKernelGGL((player_value_kernel<SRC>), dim3(grid), dim3(256), 0, stream, in, n, a, s.keys, s.idx,
                           s.s_val, s.s_ts, s.cand, s.sc);
        if (!a.absolute)
            hipLaunchKernelGGL(player_walk_kernel, dim3(grid), dim3(256), 0, stream, n, a, s.keys, s.idx, s.s_ts,
                               s.cand, s.sc);
    }
    hipLaunchKernelGGL(player_bounds_kernel, dim3((a.units + 1u + 255u) / 256u), dim3(256), 0, stream, n, a, s.keys);
    temp_bytes = s.temp_bytes;
    e = hipcub::DeviceScan::InclusiveScan(s.temp, temp_bytes, (const uint32_t *)s.cand, s.cur, hipcub::Max(), (int)m,
                                          stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(player_term_kernel, dim3(grid_m), dim3(256), 0, stream, m, a, f0, s.cur, s.term);
    temp_bytes = s.temp_bytes;
    e = hipcub::DeviceScan::InclusiveScan(s.temp, temp_bytes, (const int64_t *)s.term, s.pmin, hipcub::Min(), (int)m,
                                          stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(player_mark_kernel, dim3(grid_m), dim3(256), 0, stream, n, final_check, a, f0, s.cur, s.pmin,
                       s.mark, s.sc);
    hipcub::TransformInputIterator<uint32_t, PlayerMarked, const uint8_t *> marked(s.mark, PlayerMarked());
    temp_bytes = s.temp_bytes;
    e = hipcub::DeviceScan::ExclusiveSum(s.temp, temp_bytes, marked, s.offs, (int)m, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(player_compact_kernel, dim3(grid_m), dim3(256), 0, stream, n, s.mark, s.offs, s.pos, s.sc);
    return hipGetLastError();
}

hipError_t player_schedule(const PlayerArgs &a, int source, const void *in, uint64_t n, int final_check, uint32_t cur0,
                           uint64_t f0, PlayerScratch &s, hipStream_t stream) {
    if (source == kSrcEvents) return player_schedule_src<kSrcEvents>(a, in, n, final_check, cur0, f0, s, stream);
    if (source == kSrcWire9) return player_schedule_src<kSrcWire9>(a, in, n, final_check, cur0, f0, s, stream);
    return player_schedule_src<kSrcWire11>(a, in, n, final_check, cur0, f0, s, stream);
}

hipError_t player_handout(const PlayerArgs &a, uint64_t n, uint64_t lim, uint64_t n_frames, void *d_frames,
                          const PlayerScratch &s, hipStream_t stream) {
    const uint64_t total = n_frames * a.units;
    if (total > 0u) {
        if (a.out_type == ADDER_PLAYER_U8) {
            const uint64_t threads = (total + 3u) / 4u;
            hipLaunchKernelGGL((player_handout_kernel<uint8_t, 4>), dim3((uint32_t)((threads + 255u) / 256u)), dim3(256),
                               0, stream, a, total, s.idx, s.s_val, s.pos, (uint8_t *)d_frames);
        } else {
            hipLaunchKernelGGL((player_handout_kernel<double, 1>), dim3((uint32_t)((total + 255u) / 256u)), dim3(256), 0,
                               stream, a, total, s.idx, s.s_val, s.pos, (double *)d_frames);
        }
    }
    if (n > 0u)
        hipLaunchKernelGGL(player_commit_kernel, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, stream, n, lim, a,
                           s.keys, s.idx, s.s_val, s.s_ts);
    return hipGetLastError();
}

hipError_t player_display(const PlayerArgs &a, void *d_frame, hipStream_t stream) {
    if (a.out_type == ADDER_PLAYER_U8) {
        hipLaunchKernelGGL(player_display_kernel, dim3((a.units + 255u) / 256u), dim3(256), 0, stream, a,
                           (uint8_t *)d_frame);
        return hipGetLastError();
    }
    return hipMemcpyAsync(d_frame, a.display, (size_t)a.units * 8u, hipMemcpyDeviceToDevice, stream);
}

}  // namespace adder
