// adder_stream_kernels.h -- between adder_stream_api.cpp and adder_stream.hip (include/adder_stream.h is the public side).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace adder {

enum StreamOp : int { kStreamPass = 0, kStreamForward = 1, kStreamInverse = 2 };

struct StreamScalars {  // device words of one call, read back once at its end
    unsigned long long bad;  // smallest index of a bad event (UINT64_MAX: none)
    unsigned long long eof;  // index of the first EOF / undecodable wire record (n: none)
};

struct StreamFold {  // the dynamic-range fold, carried from call to call
    double min;                  // min_intensity (main.rs:75)
    unsigned long long max_bits;  // max_intensity as its bit pattern (non-negative doubles order as integers)
    unsigned long long count;     // events folded
};

// One step of the fold as a function on `min`: f(m) = m == 0 ? 0 : (is_const ? v : min(m, v)).
struct StreamMinOp {
    double v;
    uint32_t is_const;
    uint32_t pad;
};

struct StreamArgs {
    uint32_t width, height, channels, units;
    uint32_t key_bits;  // radix bits of a unit key; key `units` marks an event that is never worked on
    uint32_t round;     // 1: the unit's time is rounded up to ref after each event (migration only)
    uint64_t ref;       // ref_interval
    uint64_t *state;    // per unit: T (forward), L (inverse) or the last raw t (info)
};

struct StreamScratch {  // per call, n entries each
    uint32_t *keys0, *keys1, *idx0, *idx1;
    uint32_t *s_t;  // sorted order: the event's t
    uint32_t *s_o;  // sorted order: the t that comes out
    void *temp;
    size_t temp_bytes;
    // info only
    uint32_t *dt;  // input order: the event's t relative to its unit's previous one (AbsoluteT)
    StreamMinOp *op, *prefix;
    StreamScalars *sc;
};

size_t stream_temp_bytes(uint64_t n);
// n <= INT32_MAX.  Queues the whole migration on `stream`; the caller reads StreamScalars afterwards.
hipError_t stream_migrate(const StreamArgs &a, int op, int source, const void *d_in, void *d_out, uint64_t n,
                          const StreamScratch &s, hipStream_t stream);
// Folds n events into *fold (device), which holds (min0, max, count) of the events before them; absolute: the
// times are made relative to a.state first.
hipError_t stream_info(const StreamArgs &a, int absolute, int source, const void *d_in, uint64_t n, double min0,
                       StreamFold *fold, const StreamScratch &s, hipStream_t stream);

}  // namespace adder
