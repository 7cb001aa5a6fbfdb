// adder_viz_player.hip -- the adder-viz player's kernels (include/adder_viz_player.h; adder-viz player/adder.rs:319-440
// over framer/driver.rs).  The shape of adder_player.hip, with the pop schedule of adder_viz_player_logic.hpp:
//   1. keys: a unit key and a row key per record (AdderEvents or 9 / 11-byte wire records); events outside the plane
//      and EOF records are noted with atomicMin; two stable radix sorts give the unit order (a unit's events together,
//      input indices ascending) and the row order (a row's events in stream order);
//   2. walk: a thread per unit run steps the unit's FramerPx chain with framer_step and leaves, per event, last_filled
//      and the last intensity (unit order) and L at the input index of every checked event;
//   3. coverage: every fill adds to the call's count of its (row, pending frame) and takes the maximum of the event
//      index there (nat_r); an inclusive maximum of L in input order gives M; an inclusive maximum of
//      (row << 32 | L + 1) in row order makes "the first event of row r with L > W + limit" one binary search;
//   4. schedule: ONE workgroup runs the period loop, rows spread over its threads, a block reduction per period and per
//      repeated pop.  Nothing waits on another workgroup;
//   5. hand-out: a thread per unit walks the popped frames in order with a cursor into the unit's run (adjacent lanes
//      write adjacent bytes of each frame); Some = carried in the pending ring, or covered by an event with index <= P_j;
//   6. commit: pending values and their Some mask for the frames not popped, counts, trackers, unit state.
// The host waits once between 4 and 5 (the pop count sizes the output and decides whether anything is committed).
// A call made with feature detection on (adder_viz_player_features.hpp) adds: an arm of the walk that leaves each
// event's u8 value and t_after by input index; the FAST candidates, a thread per event, before the schedule; behind it
// the period-start mask, a scan and the feature records with the frames_written of their period; a cursor through the
// call's cross stamps in the hand-out (whenever the popped intervals hold features); the plane in the commit.  The host
// then waits once more, to read the features back before the crosses go up.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include "../../include/adder_viz_player.h"
#include "adder_framer_features.hpp"
#include "adder_viz_player_features.hpp"
#include "adder_viz_player_kernels.h"
#include "adder_viz_player_logic.hpp"
#include "adder_wire.hpp"

namespace adder {

__global__ void viz_init_kernel(VizScalars *sc, uint64_t n) {
    sc->bad = ~0ull;
    sc->eof = n;
    sc->status = 0u;
    sc->n_pops = 0u;
    sc->overflow = 0u;
    sc->w_end = 0;
    sc->m_end = -1;
    sc->n_feat = 0u;
}

template <int SRC>
__global__ __launch_bounds__(256) void viz_keys_kernel(const void *__restrict__ in, uint64_t n, VizArgs a,
                                                       uint32_t *__restrict__ ukeys, uint32_t *__restrict__ uidx,
                                                       uint32_t *__restrict__ rkeys, uint32_t *__restrict__ ridx,
                                                       int32_t *__restrict__ l_in, VizScalars *sc) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const WireEv e = wire_load<SRC>(in, i);
    uint32_t uk = a.units, rk = a.height;
    if (e.end) {
        atomicMin(&sc->eof, (unsigned long long)i);
    } else if (e.x < a.width && e.y < a.height && e.c < a.channels) {
        uk = (e.y * a.width + e.x) * a.channels + e.c;
        rk = e.y;
    } else {
        atomicMin(&sc->bad, (unsigned long long)i);
    }
    ukeys[i] = uk;
    uidx[i] = (uint32_t)i;
    rkeys[i] = rk;
    ridx[i] = (uint32_t)i;
    l_in[i] = -1;
}

// A thread per run: the unit's chain, event by event (framer_step), from the carried FramerPx.  DET: the arm of a call
// made with detection on also leaves, by input index, the unit's u8 value after the event and the t that
// ingest_event_for_chunk left in it (framer_feature_step).
template <int SRC, bool DET>
__global__ __launch_bounds__(256) void viz_walk_kernel(const void *__restrict__ in, uint64_t n, VizArgs a, int32_t w0,
                                                       const uint32_t *__restrict__ ukeys,
                                                       const uint32_t *__restrict__ uidx, int32_t *__restrict__ s_l,
                                                       uint8_t *__restrict__ s_val, FramerPx *__restrict__ s_px,
                                                       int32_t *__restrict__ l_in, uint8_t *__restrict__ val_in,
                                                       uint32_t *__restrict__ t_after, VizScalars *sc) {
    const uint64_t j0 = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j0 >= n) return;
    const uint32_t u = ukeys[j0];
    if (u >= a.units || (j0 > 0u && ukeys[j0 - 1] == u)) return;
    const uint64_t lim = wire_limit(sc->bad, sc->eof);
    FramerPx p = a.px[u];
    bool overflow = false, deep = false;
    const int64_t past_ring = (int64_t)w0 + (int64_t)a.ring;
    for (uint64_t j = j0; j < n && ukeys[j] == u; ++j) {
        const uint32_t i = uidx[j];
        if (i >= lim) break;
        const WireEv e = wire_load<SRC>(in, i);
        const bool checked = !(a.k.abs_t && p.ts >= (uint64_t)e.t);
        int32_t from = 0, to = 0;
        bool fills;
        if (DET) {
            const FramerFeatureStep o = framer_feature_step(p, e.d, e.t, a.k);
            fills = o.fills;
            to = o.to;
            overflow = overflow || o.overflow;
            val_in[i] = (uint8_t)o.val8;
            t_after[i] = o.t_after;
        } else {
            fills = framer_step(p, e.d, e.t, a.k, from, to, overflow);
        }
        if (fills && (int64_t)to >= past_ring) deep = true;
        s_l[j] = p.lastf;
        s_val[j] = (uint8_t)p.lasti;
        if (checked) l_in[i] = p.lastf;
    }
    s_px[j0] = p;
    if (overflow) atomicOr(&sc->status, kVizStatusRange);
    if (deep) atomicOr(&sc->status, kVizStatusDepth);
}

// The fill range of the event at unit-order position j: (from, to], empty when from == to.
__device__ __forceinline__ void viz_range(const VizArgs &a, uint64_t j, uint32_t u, const uint32_t *__restrict__ ukeys,
                                          const int32_t *__restrict__ s_l, int32_t &from, int32_t &to) {
    from = (j > 0u && ukeys[j - 1] == u) ? s_l[j - 1] : a.px[u].lastf;
    to = s_l[j];
}

__global__ __launch_bounds__(256) void viz_coverage_kernel(uint64_t n, VizArgs a, int32_t w0,
                                                           const uint32_t *__restrict__ ukeys,
                                                           const uint32_t *__restrict__ uidx,
                                                           const int32_t *__restrict__ s_l,
                                                           uint32_t *__restrict__ cnt_call,
                                                           int32_t *__restrict__ nat_call, const VizScalars *sc) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j >= n) return;
    const uint32_t u = ukeys[j];
    if (u >= a.units) return;
    const uint32_t i = uidx[j];
    if (i >= wire_limit(sc->bad, sc->eof)) return;
    int32_t from, to;
    viz_range(a, j, u, ukeys, s_l, from, to);
    const uint32_t r = u / a.row_units;
    const int64_t past_ring = (int64_t)w0 + (int64_t)a.ring;  // deeper fills are reported, not counted
    int64_t f = (int64_t)from + 1;
    if (f < (int64_t)w0) f = w0;  // frames popped before this call: late
    for (; f <= (int64_t)to && f < past_ring; ++f) {
        const size_t at = (size_t)r * a.ring + (size_t)(f % (int64_t)a.ring);
        atomicAdd(&cnt_call[at], 1u);
        atomicMax(&nat_call[at], (int32_t)i);
    }
}

__global__ __launch_bounds__(256) void viz_comb_kernel(uint64_t n, const uint32_t *__restrict__ rkeys,
                                                       const uint32_t *__restrict__ ridx,
                                                       const int32_t *__restrict__ l_in,
                                                       unsigned long long *__restrict__ comb_in) {
    const uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (p >= n) return;
    comb_in[p] = ((unsigned long long)rkeys[p] << 32) | (unsigned long long)(uint32_t)(l_in[ridx[p]] + 1);
}

// run_lo[u] = the first unit-order position whose key is >= u, for u in 0..=units
__global__ __launch_bounds__(256) void viz_bounds_kernel(uint64_t n, VizArgs a, const uint32_t *__restrict__ ukeys) {
    const uint32_t u = blockIdx.x * 256u + threadIdx.x;
    if (u > a.units) return;
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (ukeys[mid] < u)
            lo = mid + 1u;
        else
            hi = mid;
    }
    a.run_lo[u] = (uint32_t)lo;
}

// the schedule's reducer on the device: one workgroup of 256, rows strided over its threads
struct VizBlockRows {
    uint32_t rows;
    long long *sh;  // 256
    __device__ __forceinline__ bool leader() const { return threadIdx.x == 0u; }
    template <class F>
    __device__ __forceinline__ int64_t max_rows(F f) const {
        int64_t m = -kVizInf;
        for (uint32_t r = threadIdx.x; r < rows; r += 256u) m = viz_max(m, f(r));
        sh[threadIdx.x] = m;
        __syncthreads();
        for (uint32_t s = 128u; s > 0u; s >>= 1) {
            if (threadIdx.x < s) sh[threadIdx.x] = viz_max(sh[threadIdx.x], sh[threadIdx.x + s]);
            __syncthreads();
        }
        const int64_t res = sh[0];
        __syncthreads();
        return res;
    }
    template <class F>
    __device__ __forceinline__ void for_rows(F f) const {
        for (uint32_t r = threadIdx.x; r < rows; r += 256u) f(r);
    }
};

__global__ __launch_bounds__(256) void viz_schedule_kernel(VizSchedIn v, int32_t *pops, uint8_t *flushed, uint8_t *done,
                                                           VizScalars *sc) {
    __shared__ long long sh[256];
    v.n = (int64_t)wire_limit(sc->bad, sc->eof);
    VizSchedOut o;
    o.pops = pops;
    o.flushed = flushed;
    o.done = done;
    o.n_pops = 0u;
    o.overflow = 0u;
    o.w_end = v.w0;
    o.m_end = v.m0;
    VizBlockRows red{v.rows, sh};
    viz_schedule(v, red, o);
    if (threadIdx.x == 0u) {
        sc->n_pops = o.n_pops;
        sc->overflow = o.overflow;
        sc->w_end = o.w_end;
        sc->m_end = o.m_end;
    }
}

// The hot path of a call that pops: n_pops * units bytes written, each once; for frame k the 64 lanes of a wave write
// 64 consecutive bytes.  Reads per unit: 8 B of run bounds, 16 B of carried state, per frame one byte of the carried
// Some mask (plus the value when set), and its run once overall (the cursor only moves forward: 4 B of L and 4 B of
// index per event, one byte of value per covering event).
// STAMPS: a second cursor runs through the unit's cross stamps (sorted by unit, then frame); the running value after
// frame k is the later of the last Some and the last stamp at or before k, and the stamp wins inside a frame.
template <bool STAMPS>
__global__ __launch_bounds__(256) void viz_handout_kernel(VizArgs a, uint64_t lim, int32_t w0, uint32_t n_pops, int form,
                                                          const uint32_t *__restrict__ uidx,
                                                          const int32_t *__restrict__ s_l,
                                                          const uint8_t *__restrict__ s_val,
                                                          const FramerPx *__restrict__ s_px,
                                                          const int32_t *__restrict__ pops,
                                                          const uint8_t *__restrict__ flushed,
                                                          const unsigned long long *__restrict__ stamps,
                                                          uint32_t n_stamps, uint8_t *__restrict__ out) {
    const uint32_t u = blockIdx.x * 256u + threadIdx.x;
    if (u >= a.units) return;
    uint32_t q = STAMPS ? viz_stamp_first(stamps, n_stamps, u) : 0u;
    const uint32_t first = a.run_lo[u], end = a.run_lo[u + 1u];
    const FramerPx old = a.px[u];
    const bool stepped = first < end && (uint64_t)uidx[first] < lim;
    const uint32_t lasti = stepped ? s_px[first].lasti : old.lasti;  // what a flush fills a None with
    uint32_t p = first;
    uint32_t cur = a.running[u];
    for (uint32_t k = 0; k < n_pops; ++k) {
        const int64_t j = (int64_t)w0 + k;
        const size_t at = (size_t)(j % (int64_t)a.ring) * a.units + u;
        bool some = a.ring_some[at] != 0u;
        uint32_t v = 0u;
        if (some) {
            v = a.ring_val[at];
        } else {
            while (p < end && (uint64_t)uidx[p] < lim && (int64_t)s_l[p] < j) ++p;
            // the event at p covers j unless j was covered before this call (then the ring spoke: late, None)
            if (p < end && (uint64_t)uidx[p] < lim && (p > first || (int64_t)old.lastf < j)) {
                some = (int64_t)uidx[p] <= (int64_t)pops[k];
                v = s_val[p];
            }
        }
        if (!some && flushed[k]) {
            some = true;
            v = lasti;
        }
        cur = viz_running_step(cur, some, v, STAMPS && viz_stamp_take(stamps, n_stamps, q, u, k));
        out[(size_t)k * a.units + u] = (uint8_t)(form == ADDER_VIZ_FRAME_RUNNING ? cur : (some ? v : 0u));
    }
    a.running[u] = (uint8_t)cur;
}

// pending values of the frames the call did not pop
__global__ __launch_bounds__(256) void viz_commit_ring_kernel(uint64_t n, uint64_t lim, VizArgs a, int32_t w_end,
                                                              const uint32_t *__restrict__ ukeys,
                                                              const uint32_t *__restrict__ uidx,
                                                              const int32_t *__restrict__ s_l,
                                                              const uint8_t *__restrict__ s_val) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j >= n) return;
    const uint32_t u = ukeys[j];
    if (u >= a.units || (uint64_t)uidx[j] >= lim) return;
    int32_t from, to;
    viz_range(a, j, u, ukeys, s_l, from, to);
    int64_t f = (int64_t)from + 1;
    if (f < (int64_t)w_end) f = w_end;
    const uint8_t v = s_val[j];
    for (; f <= (int64_t)to; ++f) {  // to < w0 + ring: the call was refused otherwise
        const size_t at = (size_t)(f % (int64_t)a.ring) * a.units + u;
        a.ring_val[at] = v;
        a.ring_some[at] = 1u;
    }
}

__global__ __launch_bounds__(256) void viz_commit_px_kernel(uint64_t n, uint64_t lim, VizArgs a,
                                                            const uint32_t *__restrict__ ukeys,
                                                            const uint32_t *__restrict__ uidx,
                                                            const FramerPx *__restrict__ s_px) {
    const uint64_t j0 = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j0 >= n) return;
    const uint32_t u = ukeys[j0];
    if (u >= a.units || (j0 > 0u && ukeys[j0 - 1] == u) || (uint64_t)uidx[j0] >= lim) return;
    a.px[u] = s_px[j0];
}

__global__ __launch_bounds__(256) void viz_commit_rows_kernel(VizArgs a, int32_t w0, int32_t w_end,
                                                              const uint32_t *__restrict__ cnt_call,
                                                              const uint8_t *__restrict__ done_new) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= a.height * a.ring) return;
    const uint32_t r = g / a.ring, slot = g - r * a.ring;
    const uint32_t s0 = (uint32_t)((int64_t)w0 % (int64_t)a.ring);
    const int64_t f = (int64_t)w0 + (int64_t)((slot + a.ring - s0) % a.ring);  // the slot's frame in [w0, w0 + ring)
    a.cnt[g] = f < (int64_t)w_end ? 0u : a.cnt[g] + cnt_call[g];
    if (slot == 0u) a.done[r] = done_new[r];
}

// ---- feature detection (launched only by calls made with detection on) ----------------------------------------------

// A thread per event in input order: driver.rs:491-494 on the plane as it stood right before the event.  A ring pixel's
// value is the one its unit's last earlier event of this call left (a search in the unit's run), or the carried plane.
// Does not depend on the schedule.
template <int SRC>
__global__ __launch_bounds__(256) void viz_candidates_kernel(const void *__restrict__ in, uint64_t n, VizArgs a,
                                                             const uint32_t *__restrict__ uidx,
                                                             const uint8_t *__restrict__ s_val, VizDetect d,
                                                             const VizScalars *sc) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    bool feature = false;
    if (i < wire_limit(sc->bad, sc->eof)) {
        const WireEv e = wire_load<SRC>(in, i);
        const bool last_valid = i > 0u ? true : d.carry_valid != 0u;
        const uint32_t last_t = i > 0u ? d.t_after[i - 1u] : d.carry_t;
        if (framer_feature_is_candidate(e.x, e.y, e.c, e.t, last_valid, last_t, a.width, a.height)) {
            feature = fast9_ring_is_feature((int)d.val_in[i], [&](uint32_t k) -> int {
                const uint32_t rx = (uint32_t)((int)e.x + fast_ring_dx(k)), ry = (uint32_t)((int)e.y + fast_ring_dy(k));
                const uint32_t ru = (ry * a.width + rx) * a.channels;  // channel 0 of the ring pixel (cv.rs:77-87)
                return (int)framer_feature_value_before(uidx, s_val, a.run_lo[ru], a.run_lo[ru + 1u], (uint32_t)i,
                                                        d.plane[ru]);
            });
        }
    }
    d.mark[i] = feature ? 1u : 0u;
}

// behind the schedule: the first event of a period is never tested
__global__ __launch_bounds__(256) void viz_feat_flag_kernel(uint64_t n, VizDetect d, const int32_t *__restrict__ pops,
                                                            const VizScalars *sc) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    d.flag[i] = (d.mark[i] != 0u && !viz_period_start(pops, sc->n_pops, (int64_t)i)) ? 1u : 0u;
}

template <int SRC>
__global__ __launch_bounds__(256) void viz_feat_store_kernel(const void *__restrict__ in, uint64_t n, int32_t w0,
                                                             VizDetect d, const int32_t *__restrict__ pops,
                                                             VizScalars *sc) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t f = d.flag[i], o = d.offs[i];
    if (i == n - 1u) sc->n_feat = o + f;
    if (f == 0u) return;
    const WireEv e = wire_load<SRC>(in, i);
    AdderFramerFeature r;
    r.index = d.index_base + i;
    r.t = e.t;  // the raw t, also in a DeltaT stream (driver.rs:446)
    r.x = (uint16_t)e.x;
    r.y = (uint16_t)e.y;
    d.feat[o] = r;
    d.feat_w[o] = w0 + (int32_t)viz_pops_before(pops, sc->n_pops, (int64_t)i);
}

// the last event of every run that counts writes the plane
__global__ __launch_bounds__(256) void viz_commit_plane_kernel(uint64_t n, uint64_t lim, VizArgs a,
                                                               const uint32_t *__restrict__ ukeys,
                                                               const uint32_t *__restrict__ uidx,
                                                               const FramerPx *__restrict__ s_px,
                                                               uint8_t *__restrict__ plane) {
    const uint64_t j0 = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j0 >= n) return;
    const uint32_t u = ukeys[j0];
    if (u >= a.units || (j0 > 0u && ukeys[j0 - 1] == u) || (uint64_t)uidx[j0] >= lim) return;
    const uint32_t v = s_px[j0].lasti;
    plane[u] = (uint8_t)(v > 255u ? 255u : v);
}

size_t viz_temp_bytes(uint64_t n) {
    size_t a = 0, b = 0, c = 0, d = 0;
    hipcub::DoubleBuffer<uint32_t> k(nullptr, nullptr), v(nullptr, nullptr);
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, a, k, v, (int)n);
    (void)hipcub::DeviceScan::InclusiveScan(nullptr, b, (const int32_t *)nullptr, (int32_t *)nullptr, hipcub::Max(), (int)n);
    (void)hipcub::DeviceScan::InclusiveScan(nullptr, c, (const unsigned long long *)nullptr, (unsigned long long *)nullptr,
                                            hipcub::Max(), (int)n);
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, d, (const uint32_t *)nullptr, (uint32_t *)nullptr, (int)n);
    if (b > a) a = b;
    if (c > a) a = c;
    if (d > a) a = d;
    return a + 256;
}

template <int SRC>
static hipError_t viz_prepare_src(const VizArgs &a, const void *in, uint64_t n, int32_t w0, int32_t m0, int has_limit,
                                  uint32_t limit, int opening, int finish, VizScratch &s, const VizDetect &det,
                                  hipStream_t stream) {
    const uint32_t grid = (uint32_t)((n + 255u) / 256u);
    const size_t cells = (size_t)a.height * a.ring;
    hipError_t e = hipMemsetAsync(s.cnt_call, 0, cells * 4u, stream);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(s.nat_call, 0xff, cells * 4u, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(viz_init_kernel, dim3(1), dim3(1), 0, stream, s.sc, n);
    s.ukeys = s.ukeys0;
    s.uidx = s.uidx0;
    s.rkeys = s.rkeys0;
    s.ridx = s.ridx0;
    if (n > 0u) {
        hipLaunchKernelGGL((viz_keys_kernel<SRC>), dim3(grid), dim3(256), 0, stream, in, n, a, s.ukeys0, s.uidx0,
                           s.rkeys0, s.ridx0, s.l_in, s.sc);
        size_t temp_bytes = s.temp_bytes;
        hipcub::DoubleBuffer<uint32_t> uk(s.ukeys0, s.ukeys1), uv(s.uidx0, s.uidx1);
        e = hipcub::DeviceRadixSort::SortPairs(s.temp, temp_bytes, uk, uv, (int)n, 0, (int)a.unit_bits, stream);
        if (e != hipSuccess) return e;
        s.ukeys = uk.Current();
        s.uidx = uv.Current();
        temp_bytes = s.temp_bytes;
        hipcub::DoubleBuffer<uint32_t> rk(s.rkeys0, s.rkeys1), rv(s.ridx0, s.ridx1);
        e = hipcub::DeviceRadixSort::SortPairs(s.temp, temp_bytes, rk, rv, (int)n, 0, (int)a.row_bits, stream);
        if (e != hipSuccess) return e;
        s.rkeys = rk.Current();
        s.ridx = rv.Current();
        if (det.plane)
            hipLaunchKernelGGL((viz_walk_kernel<SRC, true>), dim3(grid), dim3(256), 0, stream, in, n, a, w0, s.ukeys,
                               s.uidx, s.s_l, s.s_val, s.s_px, s.l_in, det.val_in, det.t_after, s.sc);
        else
            hipLaunchKernelGGL((viz_walk_kernel<SRC, false>), dim3(grid), dim3(256), 0, stream, in, n, a, w0, s.ukeys,
                               s.uidx, s.s_l, s.s_val, s.s_px, s.l_in, (uint8_t *)nullptr, (uint32_t *)nullptr, s.sc);
        hipLaunchKernelGGL(viz_coverage_kernel, dim3(grid), dim3(256), 0, stream, n, a, w0, s.ukeys, s.uidx, s.s_l,
                           s.cnt_call, s.nat_call, s.sc);
        hipLaunchKernelGGL(viz_comb_kernel, dim3(grid), dim3(256), 0, stream, n, s.rkeys, s.ridx, s.l_in, s.comb_in);
        temp_bytes = s.temp_bytes;
        e = hipcub::DeviceScan::InclusiveScan(s.temp, temp_bytes, (const int32_t *)s.l_in, s.pm, hipcub::Max(), (int)n,
                                              stream);
        if (e != hipSuccess) return e;
        temp_bytes = s.temp_bytes;
        e = hipcub::DeviceScan::InclusiveScan(s.temp, temp_bytes, (const unsigned long long *)s.comb_in, s.comb,
                                              hipcub::Max(), (int)n, stream);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(viz_bounds_kernel, dim3((a.units + 1u + 255u) / 256u), dim3(256), 0, stream, n, a, s.ukeys);
    if (det.plane && n > 0u)
        hipLaunchKernelGGL((viz_candidates_kernel<SRC>), dim3(grid), dim3(256), 0, stream, in, n, a, s.uidx, s.s_val, det,
                           s.sc);
    VizSchedIn v{};
    v.n = 0;  // the kernel takes it from the scalars
    v.n_all = (int64_t)n;
    v.comb = s.comb;
    v.ridx = s.ridx;
    v.pm = s.pm;
    v.cnt_carry = a.cnt;
    v.cnt_call = s.cnt_call;
    v.nat_call = s.nat_call;
    v.done_carry = a.done;
    v.rows = a.height;
    v.row_units = a.row_units;
    v.ring = a.ring;
    v.w0 = w0;
    v.m0 = m0;
    v.has_limit = has_limit;
    v.limit = limit;
    v.opening = opening;
    v.finish = finish;
    v.max_pops = a.ring + 1u;
    hipLaunchKernelGGL(viz_schedule_kernel, dim3(1), dim3(256), 0, stream, v, s.pops, s.flushed, s.done_new, s.sc);
    if (det.plane && n > 0u) {
        hipLaunchKernelGGL(viz_feat_flag_kernel, dim3(grid), dim3(256), 0, stream, n, det, s.pops, s.sc);
        size_t temp_bytes = s.temp_bytes;
        const hipError_t e2 = hipcub::DeviceScan::ExclusiveSum(s.temp, temp_bytes, (const uint32_t *)det.flag, det.offs,
                                                               (int)n, stream);
        if (e2 != hipSuccess) return e2;
        hipLaunchKernelGGL((viz_feat_store_kernel<SRC>), dim3(grid), dim3(256), 0, stream, in, n, w0, det, s.pops, s.sc);
    }
    return hipGetLastError();
}

hipError_t viz_prepare(const VizArgs &a, int source, const void *in, uint64_t n, int32_t w0, int32_t m0, int has_limit,
                       uint32_t limit, int opening, int finish, VizScratch &s, const VizDetect &det, hipStream_t stream) {
    if (source == kSrcEvents)
        return viz_prepare_src<kSrcEvents>(a, in, n, w0, m0, has_limit, limit, opening, finish, s, det, stream);
    if (source == kSrcWire9)
        return viz_prepare_src<kSrcWire9>(a, in, n, w0, m0, has_limit, limit, opening, finish, s, det, stream);
    return viz_prepare_src<kSrcWire11>(a, in, n, w0, m0, has_limit, limit, opening, finish, s, det, stream);
}

hipError_t viz_handout_commit(const VizArgs &a, uint64_t n, uint64_t lim, int32_t w0, uint32_t n_pops, int form,
                              uint8_t *d_frames, const VizScratch &s, const unsigned long long *stamps,
                              uint32_t n_stamps, const VizDetect &det, hipStream_t stream) {
    const uint32_t grid = (uint32_t)((n + 255u) / 256u);
    const int32_t w_end = w0 + (int32_t)n_pops;
    if (n_pops > 0u) {
        if (n_stamps > 0u)
            hipLaunchKernelGGL(viz_handout_kernel<true>, dim3((a.units + 255u) / 256u), dim3(256), 0, stream, a, lim, w0,
                               n_pops, form, s.uidx, s.s_l, s.s_val, s.s_px, s.pops, s.flushed, stamps, n_stamps, d_frames);
        else
            hipLaunchKernelGGL(viz_handout_kernel<false>, dim3((a.units + 255u) / 256u), dim3(256), 0, stream, a, lim, w0,
                               n_pops, form, s.uidx, s.s_l, s.s_val, s.s_px, s.pops, s.flushed,
                               (const unsigned long long *)nullptr, 0u, d_frames);
        // the popped frames' slots serve frames w0 + ring .. from here on: no Some left in them (n_pops <= ring)
        const uint32_t s0 = (uint32_t)(w0 % (int32_t)a.ring);
        const uint32_t head = n_pops < a.ring - s0 ? n_pops : a.ring - s0;
        hipError_t e = hipMemsetAsync(a.ring_some + (size_t)s0 * a.units, 0, (size_t)head * a.units, stream);
        if (e != hipSuccess) return e;
        if (n_pops > head) {
            e = hipMemsetAsync(a.ring_some, 0, (size_t)(n_pops - head) * a.units, stream);
            if (e != hipSuccess) return e;
        }
    }
    if (n > 0u) {
        hipLaunchKernelGGL(viz_commit_ring_kernel, dim3(grid), dim3(256), 0, stream, n, lim, a, w_end, s.ukeys, s.uidx,
                           s.s_l, s.s_val);
        hipLaunchKernelGGL(viz_commit_px_kernel, dim3(grid), dim3(256), 0, stream, n, lim, a, s.ukeys, s.uidx, s.s_px);
        if (det.plane)
            hipLaunchKernelGGL(viz_commit_plane_kernel, dim3(grid), dim3(256), 0, stream, n, lim, a, s.ukeys, s.uidx,
                               s.s_px, det.plane);
    }
    hipLaunchKernelGGL(viz_commit_rows_kernel, dim3((a.height * a.ring + 255u) / 256u), dim3(256), 0, stream, a, w0, w_end,
                       s.cnt_call, s.done_new);
    return hipGetLastError();
}

}  // namespace adder
