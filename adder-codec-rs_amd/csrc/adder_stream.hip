// adder_stream.hip -- time-mode migration and the adder-info fold (include/adder_stream.h;
// adder-codec-rs/src/utils/stream_migration.rs:32-88, adder-info/src/main.rs:74-121).
//
// The shape of adder_dvs.hip without the logarithm:
//   1. keys: unit index per event (decoded from AdderEvents or 9 / 11-byte wire records), out-of-plane and EOF
//      records noted with atomicMin; a stable radix sort on ceil(log2(units + 1)) bits brings a unit's events
//      together; a gather puts their times in sorted order;
//   2. forward (DeltaT -> AbsoluteT): a thread per run chains T += t and the round-up, u64 adds and one division;
//      inverse (AbsoluteT -> DeltaT) and AbsoluteT info: a thread per sorted event, its predecessor is its neighbour
//      (or the state plane for the head of a run) -- no chain;
//   3. emit: a thread per sorted event writes the record at its INPUT index and, for the last event of its run in
//      front of the first bad / EOF index, the unit's state.  The state after an event follows from that event
//      alone, so a failed call commits exactly the events before the bad index without a second set of planes.
// The info fold runs in INPUT order: every event is a function on `min` (StreamMinOp), an exclusive scan composes
// them, a map offers each intensity to `max` unless it lowered `min`, a block reduction and one atomicMax per block
// keep the maximum.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include "../../include/adder_stream.h"
#include "adder_stream_kernels.h"
#include "adder_wire.hpp"

namespace adder {

// wire_load, but the 11-byte arm addresses d and t through wire11_t_offset, as stream_store does: the copy kernel loads
// and stores the same record, and with one offset for both its wire-11 call measured 79 us against 85 us with the
// branch of wire_load (1 << 22 records on 640x480x3; profiles/stream_wire11_timing.json).  Same result, byte for byte.
template <int SRC>
__device__ __forceinline__ WireEv stream_load(const void *in, uint64_t i) {
    if (SRC != kSrcWire11) return wire_load<SRC>(in, i);
    const uint8_t *p = (const uint8_t *)in + i * 11u;
    const uint32_t tag = p[4];
    WireEv e;
    e.x = wire_be16(p);
    e.y = wire_be16(p + 2);
    e.c = tag == 1u ? p[5] : 0u;
    e.d = p[wire11_t_offset(tag) - 1u];
    e.t = wire_be32(p + wire11_t_offset(tag));
    e.end = tag > 1u || (e.x == 0xffffu && e.y == 0xffffu);
    return e;
}

// record i of `in` -> record i of `out` with its time replaced (out == in allowed: one thread owns the record).
// The WHOLE record: every byte other than the four of t is the input's, whichever tag -- a None record's t ends at
// byte 9 and its byte 10 is carried like the rest.
template <int SRC>
__device__ __forceinline__ void stream_store(const void *in, void *out, uint64_t i, uint32_t t) {
    if (SRC == kSrcEvents) {
        AdderEvent ev = ((const AdderEvent *)in)[i];
        ev.t = t;
        ((AdderEvent *)out)[i] = ev;
    } else {
        const uint32_t rb = SRC == kSrcWire9 ? 9u : 11u;
        const uint8_t *p = (const uint8_t *)in + i * rb;
        uint8_t *q = (uint8_t *)out + i * rb;
        const uint32_t off = SRC == kSrcWire9 ? 5u : wire11_t_offset(p[4]);
        if (q != p) {
            for (uint32_t k = 0; k < off; ++k) q[k] = p[k];
            for (uint32_t k = off + 4u; k < rb; ++k) q[k] = p[k];
        }
        q[off] = (uint8_t)(t >> 24);
        q[off + 1u] = (uint8_t)(t >> 16);
        q[off + 2u] = (uint8_t)(t >> 8);
        q[off + 3u] = (uint8_t)t;
    }
}

__global__ void stream_init_kernel(StreamScalars *sc, uint64_t n) {
    sc->bad = ~0ull;
    sc->eof = n;
}

// keys == nullptr: only the bad / EOF indices are wanted (no sort follows)
template <int SRC>
__global__ __launch_bounds__(256) void stream_keys_kernel(const void *__restrict__ in, uint64_t n, StreamArgs a,
                                                          uint32_t *__restrict__ keys, uint32_t *__restrict__ idx,
                                                          StreamScalars *sc) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const WireEv e = stream_load<SRC>(in, i);
    uint32_t key = a.units;  // sorted behind every unit, never worked on
    if (e.end) {
        atomicMin(&sc->eof, (unsigned long long)i);
    } else if (e.x < a.width && e.y < a.height && e.c < a.channels) {
        key = (e.y * a.width + e.x) * a.channels + e.c;
    } else {
        atomicMin(&sc->bad, (unsigned long long)i);
    }
    if (keys) {
        keys[i] = key;
        idx[i] = (uint32_t)i;
    }
}

template <int SRC>
__global__ __launch_bounds__(256) void stream_gather_kernel(const void *__restrict__ in, uint64_t n, StreamArgs a,
                                                            const uint32_t *__restrict__ keys,
                                                            const uint32_t *__restrict__ idx,
                                                            uint32_t *__restrict__ s_t) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j >= n || keys[j] >= a.units) return;
    s_t[j] = stream_load<SRC>(in, idx[j]).t;
}

// migrate_v2's loop body for one unit: T += t; t_out = T; T rounded up (stream_migration.rs:59-83)
__global__ __launch_bounds__(256) void stream_forward_kernel(uint64_t n, StreamArgs a,
                                                             const uint32_t *__restrict__ keys,
                                                             const uint32_t *__restrict__ idx,
                                                             const uint32_t *__restrict__ s_t,
                                                             uint32_t *__restrict__ s_o, StreamScalars *sc) {
    const uint64_t j0 = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j0 >= n) return;
    const uint32_t u = keys[j0];
    if (u >= a.units || (j0 > 0u && keys[j0 - 1] == u)) return;  // a thread per run of one unit
    const uint64_t lim = wire_limit(sc->bad, sc->eof);  // as the keys kernel left it; an overflow below can only lower it
    uint64_t T = a.state[u];
    for (uint64_t j = j0; j < n && keys[j] == u; ++j) {
        const uint32_t i = idx[j];
        if (i >= lim) break;
        T += s_t[j];
        if (T > 0xffffffffull) {
            atomicMin(&sc->bad, (unsigned long long)i);
            break;
        }
        s_o[j] = (uint32_t)T;
        if (a.round) T = wire_round_up(T, a.ref);
    }
}

// dt = t - L, L = the predecessor's time (rounded up in a migration, raw in adder-info)
__global__ __launch_bounds__(256) void stream_inverse_kernel(uint64_t n, StreamArgs a,
                                                             const uint32_t *__restrict__ keys,
                                                             const uint32_t *__restrict__ idx,
                                                             const uint32_t *__restrict__ s_t,
                                                             uint32_t *__restrict__ s_o, StreamScalars *sc) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j >= n) return;
    const uint32_t u = keys[j];
    if (u >= a.units) return;
    uint64_t L;
    if (j == 0u || keys[j - 1] != u) {
        L = a.state[u];
    } else {
        L = s_t[j - 1];
        if (a.round) L = wire_round_up(L, a.ref);
    }
    const uint64_t t = s_t[j];
    if (t < L)
        atomicMin(&sc->bad, (unsigned long long)idx[j]);
    else
        s_o[j] = (uint32_t)(t - L);
}

// The record (OUT_RECORDS) or the relative time (dt) at the event's input index, and the state of a unit whose
// last event in front of the limit this is: forward, round_up(t_out); inverse / info, round_up(t_in) / t_in.
template <int SRC, bool OUT_RECORDS>
__global__ __launch_bounds__(256) void stream_emit_kernel(const void *in, void *out, uint32_t *__restrict__ dt,
                                                          uint64_t n, StreamArgs a, int forward,
                                                          const uint32_t *__restrict__ keys,
                                                          const uint32_t *__restrict__ idx,
                                                          const uint32_t *__restrict__ s_t,
                                                          const uint32_t *__restrict__ s_o, const StreamScalars *sc) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j >= n) return;
    const uint32_t u = keys[j];
    if (u >= a.units) return;
    const uint64_t lim = wire_limit(sc->bad, sc->eof);
    const uint32_t i = idx[j];
    if (i >= lim) return;
    const uint32_t o = s_o[j];
    if (OUT_RECORDS)
        stream_store<SRC>(in, out, i, o);
    else
        dt[i] = o;
    if (j + 1u == n || keys[j + 1] != u || idx[j + 1] >= lim) {  // idx ascends within a run (stable sort)
        const uint64_t base = forward ? o : s_t[j];
        a.state[u] = a.round ? wire_round_up(base, a.ref) : base;
    }
}

template <int SRC>
__global__ __launch_bounds__(256) void stream_copy_kernel(const void *in, void *out, uint64_t n,
                                                          const StreamScalars *sc) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n || i >= wire_limit(sc->bad, sc->eof)) return;
    stream_store<SRC>(in, out, i, stream_load<SRC>(in, i).t);
}

// ---- the dynamic-range fold --------------------------------------------------------------------------------------

// g after f
struct StreamCompose {
    __host__ __device__ __forceinline__ StreamMinOp operator()(const StreamMinOp &f, const StreamMinOp &g) const {
        if (f.is_const && f.v == 0.0) return f;  // min == 0 is for good
        if (g.is_const) return g;
        StreamMinOp r = f;
        r.v = g.v < f.v ? g.v : f.v;
        return r;
    }
};

__device__ __forceinline__ double stream_apply(const StreamMinOp &f, double m) {
    if (m == 0.0) return 0.0;
    if (f.is_const) return f.v;
    return f.v < m ? f.v : m;
}

// event_to_intensity (scale_intensity.rs:262-270) and the match of main.rs:102-121 as a StreamMinOp
template <int SRC>
__global__ __launch_bounds__(256) void stream_fold_prep_kernel(const void *__restrict__ in, uint64_t n,
                                                               const uint32_t *__restrict__ dt,
                                                               const StreamScalars *sc, StreamMinOp *__restrict__ op) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    StreamMinOp f;
    f.v = __longlong_as_double(0x7ff0000000000000ll);  // min(m, +inf): the identity
    f.is_const = 0u;
    f.pad = 0u;
    if (i < wire_limit(sc->bad, sc->eof)) {
        const WireEv e = stream_load<SRC>(in, i);
        const uint32_t t = dt ? dt[i] : e.t;
        if (e.d == 255u) {
            // D_EMPTY: ignored
        } else if (e.d > 128u) {  // intensity 0.0 < min: min = 0.0
            f.v = 0.0;
            f.is_const = 1u;
        } else if (e.d == 128u) {  // intensity 0.0 < min: min = 1.0 / t (+inf for t == 0)
            f.v = 1.0 / (double)t;
            f.is_const = 1u;
        } else {
            const double p = __longlong_as_double((long long)(1023u + e.d) << 52);  // 2^d
            f.v = t == 0u ? p : p / (double)t;
        }
    }
    op[i] = f;
}

__global__ __launch_bounds__(256) void stream_fold_map_kernel(uint64_t n, const StreamMinOp *__restrict__ op,
                                                              const StreamMinOp *__restrict__ prefix,
                                                              const StreamScalars *sc, StreamFold *fold) {
    using Reduce = hipcub::BlockReduce<unsigned long long, 256>;
    __shared__ typename Reduce::TempStorage tmp;
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint64_t lim = wire_limit(sc->bad, sc->eof);
    unsigned long long cand = 0ull;
    if (i < n && i < lim) {
        const StreamMinOp f = op[i];
        const double m = prefix[i].v;  // the scan starts from a constant, so every prefix is one
        // an intensity that does not lower min is offered to max; 0.0 (d >= 128) never raises it
        if (!f.is_const && f.v < __longlong_as_double(0x7ff0000000000000ll) && !(f.v < m))
            cand = (unsigned long long)__double_as_longlong(f.v);
        if (i + 1u == lim) {
            fold->min = stream_apply(f, m);
            fold->count += lim;
        }
    }
    const unsigned long long best = Reduce(tmp).Reduce(cand, hipcub::Max());
    // max only grows, so a plain look first keeps all but a few blocks off the one word
    if (threadIdx.x == 0u && best > *(volatile unsigned long long *)&fold->max_bits) atomicMax(&fold->max_bits, best);
}

size_t stream_temp_bytes(uint64_t n) {
    size_t a = 0, b = 0;
    hipcub::DoubleBuffer<uint32_t> k(nullptr, nullptr), v(nullptr, nullptr);
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, a, k, v, (int)n);
    StreamMinOp init{};
    (void)hipcub::DeviceScan::ExclusiveScan(nullptr, b, (const StreamMinOp *)nullptr, (StreamMinOp *)nullptr,
                                            StreamCompose(), init, (int)n);
    return (a > b ? a : b) + 256;
}

template <int SRC>
static hipError_t stream_migrate_src(const StreamArgs &a, int op, const void *in, void *out, uint64_t n,
                                     const StreamScratch &s, hipStream_t stream) {
    const dim3 grid((uint32_t)((n + 255u) / 256u)), block(256);
    hipLaunchKernelGGL(stream_init_kernel, dim3(1), dim3(1), 0, stream, s.sc, n);
    if (op == kStreamPass) {
        hipLaunchKernelGGL((stream_keys_kernel<SRC>), grid, block, 0, stream, in, n, a, (uint32_t *)nullptr,
                           (uint32_t *)nullptr, s.sc);
        if (out != in) hipLaunchKernelGGL((stream_copy_kernel<SRC>), grid, block, 0, stream, in, out, n, s.sc);
        return hipGetLastError();
    }
    hipLaunchKernelGGL((stream_keys_kernel<SRC>), grid, block, 0, stream, in, n, a, s.keys0, s.idx0, s.sc);
    hipcub::DoubleBuffer<uint32_t> k(s.keys0, s.keys1), v(s.idx0, s.idx1);
    size_t temp_bytes = s.temp_bytes;
    hipError_t e = hipcub::DeviceRadixSort::SortPairs(s.temp, temp_bytes, k, v, (int)n, 0, (int)a.key_bits, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((stream_gather_kernel<SRC>), grid, block, 0, stream, in, n, a, k.Current(), v.Current(), s.s_t);
    if (op == kStreamForward)
        hipLaunchKernelGGL(stream_forward_kernel, grid, block, 0, stream, n, a, k.Current(), v.Current(), s.s_t, s.s_o,
                           s.sc);
    else
        hipLaunchKernelGGL(stream_inverse_kernel, grid, block, 0, stream, n, a, k.Current(), v.Current(), s.s_t, s.s_o,
                           s.sc);
    hipLaunchKernelGGL((stream_emit_kernel<SRC, true>), grid, block, 0, stream, in, out, (uint32_t *)nullptr, n, a,
                       op == kStreamForward ? 1 : 0, k.Current(), v.Current(), s.s_t, s.s_o, s.sc);
    return hipGetLastError();
}

hipError_t stream_migrate(const StreamArgs &a, int op, int source, const void *in, void *out, uint64_t n,
                          const StreamScratch &s, hipStream_t stream) {
    if (n == 0u) return hipSuccess;
    if (source == kSrcEvents) return stream_migrate_src<kSrcEvents>(a, op, in, out, n, s, stream);
    if (source == kSrcWire9) return stream_migrate_src<kSrcWire9>(a, op, in, out, n, s, stream);
    return stream_migrate_src<kSrcWire11>(a, op, in, out, n, s, stream);
}

template <int SRC>
static hipError_t stream_info_src(const StreamArgs &a, int absolute, const void *in, uint64_t n, double min0,
                                  StreamFold *fold, const StreamScratch &s, hipStream_t stream) {
    const dim3 grid((uint32_t)((n + 255u) / 256u)), block(256);
    size_t temp_bytes = s.temp_bytes;
    hipLaunchKernelGGL(stream_init_kernel, dim3(1), dim3(1), 0, stream, s.sc, n);
    if (absolute) {
        hipLaunchKernelGGL((stream_keys_kernel<SRC>), grid, block, 0, stream, in, n, a, s.keys0, s.idx0, s.sc);
        hipcub::DoubleBuffer<uint32_t> k(s.keys0, s.keys1), v(s.idx0, s.idx1);
        hipError_t e = hipcub::DeviceRadixSort::SortPairs(s.temp, temp_bytes, k, v, (int)n, 0, (int)a.key_bits, stream);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((stream_gather_kernel<SRC>), grid, block, 0, stream, in, n, a, k.Current(), v.Current(),
                           s.s_t);
        hipLaunchKernelGGL(stream_inverse_kernel, grid, block, 0, stream, n, a, k.Current(), v.Current(), s.s_t, s.s_o,
                           s.sc);
        hipLaunchKernelGGL((stream_emit_kernel<SRC, false>), grid, block, 0, stream, in, (void *)nullptr, s.dt, n, a, 0,
                           k.Current(), v.Current(), s.s_t, s.s_o, s.sc);
    } else {
        hipLaunchKernelGGL((stream_keys_kernel<SRC>), grid, block, 0, stream, in, n, a, (uint32_t *)nullptr,
                           (uint32_t *)nullptr, s.sc);
    }
    hipLaunchKernelGGL((stream_fold_prep_kernel<SRC>), grid, block, 0, stream, in, n,
                       absolute ? (const uint32_t *)s.dt : (const uint32_t *)nullptr, s.sc, s.op);
    StreamMinOp init;
    init.v = min0;
    init.is_const = 1u;
    init.pad = 0u;
    temp_bytes = s.temp_bytes;
    hipError_t e = hipcub::DeviceScan::ExclusiveScan(s.temp, temp_bytes, (const StreamMinOp *)s.op, s.prefix,
                                                     StreamCompose(), init, (int)n, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(stream_fold_map_kernel, grid, block, 0, stream, n, s.op, s.prefix, s.sc, fold);
    return hipGetLastError();
}

hipError_t stream_info(const StreamArgs &a, int absolute, int source, const void *in, uint64_t n, double min0,
                       StreamFold *fold, const StreamScratch &s, hipStream_t stream) {
    if (n == 0u) return hipSuccess;
    if (source == kSrcEvents) return stream_info_src<kSrcEvents>(a, absolute, in, n, min0, fold, s, stream);
    if (source == kSrcWire9) return stream_info_src<kSrcWire9>(a, absolute, in, n, min0, fold, s, stream);
    return stream_info_src<kSrcWire11>(a, absolute, in, n, min0, fold, s, stream);
}

}  // namespace adder
