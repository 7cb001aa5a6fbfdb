// adder_davis.hip -- one DAVIS packet -> sparse steps on the device (include/adder_davis.h; davis.rs:233-598, :775-864).
//
// The shape of adder_prophesee.hip: a pixel's events form a serial chain (last ln is multiplied event after event),
// pixels are independent.  The held `after` events of the previous packet and this packet's `before` events are one
// list of n events, held first.
//   1. chunk keys: (list, row chunk) per event, 8 for an event that fails its time checks or lies outside the plane
//      (the latter noted with atomicMin for `before` and for the new `after` events); a stable 4-bit radix sort gives the
//      step order -- lists one after the other, the four chunks one after the other, arrival order inside a chunk;
//   2. pixel keys in step order; a stable radix sort brings a pixel's events together, still in step order;
//   3. gather: the sorted events side by side as {t, step rank, on, last of its pixel}, so that the walk reads one
//      sequential 16-byte record per event and can load the next one ahead of the chain's exps;
//      walk: a lane per run keeps the pixel's last ln / last ts in registers, evaluates the exps on the chain and writes
//      each event's 0 or 2 steps into the event's two slots (by step rank), then the pixel's state into the work planes;
//   4. an exclusive scan of the counts in step order places the steps; a lane per event copies them (coalesced);
//   5. gaps: a lane per pixel on the work planes, 0 / 1 counts, scan, compaction behind the events' steps;
//   6. frame: a lane per pixel -- the frame check, image_8u, the pixel's step behind the gaps', last ln, last ts.
// The sorts, the scans and the compaction of step 4 are adder_chain.hip's, shared with adder_prophesee.hip.
// Everything works on a copy of the state planes: the host commits by swapping the planes once it has read the
// bad-event and bad-frame words, so a refused push changes nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "adder_davis_kernels.h"
#include "adder_davis_logic.hpp"

namespace adder {

struct DavisEv {
    int64_t t;
    uint32_t x, y;
    bool on;
};

// {i64 t; u16 x, y; u8 on; pad[3]} as two 8-byte words
__device__ __forceinline__ DavisEv davis_load(const AdderDavisEvent *ev, uint64_t i) {
    const unsigned long long *w = (const unsigned long long *)ev + 2u * i;
    const unsigned long long w0 = w[0], w1 = w[1];
    DavisEv e;
    e.t = (int64_t)w0;
    e.x = (uint32_t)(w1 & 0xffffu);
    e.y = (uint32_t)((w1 >> 16) & 0xffffu);
    e.on = ((w1 >> 32) & 0xffu) != 0u;
    return e;
}

// event `src` of the list: the held events, then `before`
__device__ __forceinline__ DavisEv davis_list_event(const DavisPacket &pk, uint64_t src) {
    return src < pk.n_held ? davis_load(pk.held, src) : davis_load(pk.before, src - pk.n_held);
}

__global__ void davis_init_scalars_kernel(DavisScalars *sc) {
    sc->bad = ~0ull;
    sc->bad_frame = ~0ull;
    sc->ev_steps = 0ull;
    sc->gap_steps = 0ull;
}

// lanes [0, n): the list's chunk keys; lanes [n, n + n_after): the bounds check of the new `after` events alone
__global__ __launch_bounds__(256) void davis_chunk_keys_kernel(DavisArgs a, DavisPacket pk, uint64_t n,
                                                               uint32_t *__restrict__ keys, uint32_t *__restrict__ idx,
                                                               DavisScalars *sc) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n + pk.n_after) return;
    if (i >= n) {
        const DavisEv e = davis_load(pk.after, i - n);
        if (e.x >= a.width || e.y >= a.height) atomicMin(&sc->bad, (unsigned long long)(pk.n_before + (i - n)));
        return;
    }
    const DavisEv e = davis_list_event(pk, i);
    const bool held = i < pk.n_held;
    uint32_t key = 8u;
    if (e.x < a.width && e.y < a.height) {
        if (davis_event_passes(e.t, pk.start, held ? pk.held_check2 : 0, pk.end_of_last))
            key = (held ? 0u : 4u) + e.y / a.chunk_h;
    } else if (!held) {
        atomicMin(&sc->bad, (unsigned long long)(i - pk.n_held));
    }
    keys[i] = key;
    idx[i] = (uint32_t)i;
}

// by step rank: the pixel of the event, `units` for one that makes no step
__global__ __launch_bounds__(256) void davis_pixel_keys_kernel(DavisArgs a, DavisPacket pk, uint64_t n,
                                                               const uint32_t *__restrict__ chunk_keys,
                                                               const uint32_t *__restrict__ order,
                                                               uint32_t *__restrict__ keys, uint32_t *__restrict__ idx) {
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (r >= n) return;
    uint32_t key = a.units;
    if (chunk_keys[r] < 8u) {
        const DavisEv e = davis_list_event(pk, order[r]);
        key = e.y * a.width + e.x;
    }
    keys[r] = key;
    idx[r] = (uint32_t)r;
}

__global__ __launch_bounds__(256) void davis_gather_kernel(DavisArgs a, DavisPacket pk, uint64_t n,
                                                           const uint32_t *__restrict__ keys,
                                                           const uint32_t *__restrict__ idx,
                                                           const uint32_t *__restrict__ order,
                                                           DavisWalkEvent *__restrict__ sorted) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j >= n) return;
    const uint32_t u = keys[j];
    if (u >= a.units) return;
    const uint32_t r = idx[j];
    const DavisEv e = davis_list_event(pk, order[r]);
    const bool last = j + 1u >= n || keys[j + 1] != u;
    DavisWalkEvent w;
    w.t = e.t;
    w.rank = r;
    w.flags = (e.on ? 1u : 0u) | (last ? 2u : 0u);
    sorted[j] = w;
}

__global__ __launch_bounds__(256) void davis_walk_kernel(DavisArgs a, DavisPacket pk, uint64_t n, DavisPlanes work,
                                                         const uint32_t *__restrict__ keys,
                                                         const uint32_t *__restrict__ idx,
                                                         const DavisWalkEvent *__restrict__ sorted,
                                                         uint32_t *__restrict__ cnt, AdderSparseStep *__restrict__ stage) {
    const uint64_t j0 = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j0 >= n) return;
    const uint32_t u = keys[j0];
    if (u >= a.units) {  // no step: the count is still defined
        cnt[idx[j0]] = 0u;
        return;
    }
    if (j0 > 0u && keys[j0 - 1] == u) return;  // a lane per run of one pixel
    const DavisConsts k = davis_consts(pk.c, a.tps, a.ref_time);
    DavisPixel px = davis_pixel(work.ts[u], work.ln[u]);
    const uint32_t x = u % a.width, y = u / a.width;
    DavisWalkEvent e = sorted[j0];
    for (uint64_t j = j0;; ++j) {
        const DavisWalkEvent next = sorted[j + 1u < n ? j + 1u : j];  // in flight while the chain's exps run
        cnt[e.rank] = davis_event_steps(px, x, y, e.t, (e.flags & 1u) != 0u, k, stage + 2u * (uint64_t)e.rank);
        if ((e.flags & 2u) != 0u || j + 1u >= n) break;
        e = next;
    }
    work.ts[u] = px.ts;
    work.ln[u] = px.ln;
}

__global__ __launch_bounds__(256) void davis_gaps_kernel(DavisArgs a, DavisPacket pk, DavisPlanes work,
                                                         uint32_t *__restrict__ gcnt, AdderSparseStep *__restrict__ gstage) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= a.units) return;
    const DavisConsts k = davis_consts(pk.c, a.tps, a.ref_time);
    double ln = work.ln[p];
    gcnt[p] = davis_gap_step(work.ts[p], ln, p % a.width, p / a.width, pk.start, k, gstage + p);
    work.ln[p] = ln;
}

__global__ __launch_bounds__(256) void davis_gap_scatter_kernel(DavisArgs a, const uint32_t *__restrict__ gcnt,
                                                                const uint32_t *__restrict__ goffs,
                                                                const AdderSparseStep *__restrict__ gstage,
                                                                AdderSparseStep *__restrict__ steps, DavisScalars *sc) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= a.units) return;
    const uint32_t c = gcnt[p], o = goffs[p];
    if (c) steps[sc->ev_steps + o] = gstage[p];
    if (p == a.units - 1u) sc->gap_steps = (unsigned long long)o + c;
}

// raw modes: steps != nullptr and the pixel's step goes behind the events' and the gaps'; Framed: img alone
__global__ __launch_bounds__(256) void davis_frame_kernel(DavisArgs a, DavisPacket pk, DavisPlanes work,
                                                          uint8_t *__restrict__ img, AdderSparseStep *__restrict__ steps,
                                                          DavisScalars *sc) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= a.units) return;
    double v = 0.0;
    if (a.mode != ADDER_DAVIS_RAW_DVS) {
        v = pk.frame[p];
        if (!davis_frame_value_ok(v)) {
            atomicMin(&sc->bad_frame, (unsigned long long)p);
            v = 0.0;  // the push is refused; nothing below depends on a refused value
        }
    }
    double ln;
    const uint8_t b = davis_frame_pixel(a.mode, v, ln);
    work.ln[p] = ln;
    if (a.mode == ADDER_DAVIS_FRAMED) {
        img[p] = b;
        return;
    }
    work.ts[p] = pk.end;
    steps[sc->ev_steps + sc->gap_steps + p] =
        davis_step(p % a.width, p / a.width, b, 0u, (float)b, davis_frame_span(a.mode, pk.start, pk.end, a.ref_time));
}

__global__ __launch_bounds__(256) void davis_flush_kernel(DavisArgs a, AdderSparseStep *__restrict__ steps) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= a.units) return;
    steps[p] = davis_step(p % a.width, p / a.width, 0u, ADDER_SPARSE_NO_SIDE | ADDER_SPARSE_FLUSH, 0.0f, 0.0f);
}

hipError_t davis_generate(const DavisArgs &a, const DavisPacket &pk, const DavisPlanes &work, const DavisScratch &s,
                          AdderSparseStep *d_steps, uint8_t *d_img, hipStream_t stream) {
    hipLaunchKernelGGL(davis_init_scalars_kernel, dim3(1), dim3(1), 0, stream, s.sc);
    const bool raw = a.mode != ADDER_DAVIS_FRAMED;
    const uint64_t n = raw ? pk.n_held + pk.n_before : 0u;
    const uint32_t pgrid = grid_of(a.units);
    const ChainScratch &c = s.chain;
    hipError_t e = hipSuccess;
    if (raw && n + pk.n_after > 0u)
        hipLaunchKernelGGL(davis_chunk_keys_kernel, dim3(grid_of(n + pk.n_after)), dim3(256), 0, stream, a, pk, n, c.keys0,
                           c.idx0, s.sc);
    if (n > 0u) {
        const uint32_t grid = grid_of(n);
        if ((e = chain_sort_pairs(c, n, 4, stream)) != hipSuccess) return e;
        // keys0 = the sorted chunk keys, idx0 = the step order; both are sorted over again below
        if ((e = hipMemcpyAsync(s.order, c.idx0, n * 4u, hipMemcpyDeviceToDevice, stream)) != hipSuccess) return e;
        if ((e = hipMemcpyAsync(c.cnt, c.keys0, n * 4u, hipMemcpyDeviceToDevice, stream)) != hipSuccess) return e;
        hipLaunchKernelGGL(davis_pixel_keys_kernel, dim3(grid), dim3(256), 0, stream, a, pk, n, c.cnt, s.order, c.keys0,
                           c.idx0);
        if ((e = chain_sort_pairs(c, n, (int)a.key_bits, stream)) != hipSuccess) return e;
        hipLaunchKernelGGL(davis_gather_kernel, dim3(grid), dim3(256), 0, stream, a, pk, n, c.keys0, c.idx0, s.order,
                           s.sorted);
        hipLaunchKernelGGL(davis_walk_kernel, dim3(grid), dim3(256), 0, stream, a, pk, n, work, c.keys0, c.idx0, s.sorted,
                           c.cnt, c.stage);
        if ((e = chain_scan_counts(c, n, &s.sc->ev_steps, stream)) != hipSuccess) return e;
        if ((e = chain_scatter(c, n, d_steps, stream)) != hipSuccess) return e;
    }
    if (raw) {
        hipLaunchKernelGGL(davis_gaps_kernel, dim3(pgrid), dim3(256), 0, stream, a, pk, work, s.gcnt, s.gstage);
        if ((e = chain_exclusive_sum(c, s.gcnt, s.goffs, a.units, stream)) != hipSuccess) return e;
        hipLaunchKernelGGL(davis_gap_scatter_kernel, dim3(pgrid), dim3(256), 0, stream, a, s.gcnt, s.goffs, s.gstage, d_steps,
                           s.sc);
    }
    hipLaunchKernelGGL(davis_frame_kernel, dim3(pgrid), dim3(256), 0, stream, a, pk, work, d_img, raw ? d_steps : nullptr,
                       s.sc);
    return hipGetLastError();
}

hipError_t davis_flush_steps(const DavisArgs &a, AdderSparseStep *d_steps, hipStream_t stream) {
    hipLaunchKernelGGL(davis_flush_kernel, dim3(grid_of(a.units)), dim3(256), 0, stream, a, d_steps);
    return hipGetLastError();
}

}  // namespace adder
