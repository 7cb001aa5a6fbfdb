// adder_dvs_kernels.h -- between adder_dvs_api.cpp and adder_dvs.hip (include/adder_dvs.h is the public side).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace adder {


struct DvsScalars {  // device words of one call, read back once at its end
    unsigned long long bad;  // smallest index of a bad event (UINT64_MAX: none)
    unsigned long long eof;  // index of the first EOF / undecodable wire record (n: none)
    unsigned long long total;  // fired events of the call (the required output count)
};

struct DvsArgs {
    uint32_t width, height, channels, units;
    uint32_t key_bits;     // radix bits of a unit key; key `units` marks an event that is never walked
    uint32_t delta_t;      // 1: DeltaT accumulation, 0: AbsoluteT rules
    uint32_t framed;       // is_framed(source_camera): times rounded up to ref_interval
    uint64_t ref;          // ref_interval
    double ref_f;          // ref_interval as f64
    double win_hi;         // ln_1p(1.0) - theta
    double win_lo;         // ln_1p(0.0) + theta
    double half;           // theta / 2.0
    // per-unit state: `cur` is read, a call's walk writes `nxt`, the commit copies the walked units back
    uint8_t *cur_init, *nxt_init;
    double *cur_ln, *nxt_ln;
    uint64_t *cur_t, *nxt_t;
};

struct DvsScratch {  // per call, n entries each unless said otherwise
    uint32_t *keys0, *keys1, *idx0, *idx1;
    double *s_ln;      // sorted order: the event's ln intensity
    uint64_t *s_td;    // sorted order: raw t | d << 32
    uint8_t *flag;     // input order: 0 none, 1 negative, 2 positive
    uint64_t *tout;    // input order: the fired event's time
    uint32_t *offs;    // input order: exclusive scan of flag != 0
    void *temp;
    size_t temp_bytes;
    DvsScalars *sc;
};

size_t dvs_temp_bytes(uint64_t n);
// n <= INT32_MAX.  Queues the whole conversion on `stream`; the caller reads DvsScalars afterwards.
hipError_t dvs_convert(const DvsArgs &a, int source, const void *d_in, uint64_t n, int out_format, void *d_out,
                       uint64_t out_cap, const DvsScratch &s, hipStream_t stream);
size_t dvs_sort_temp_bytes(uint64_t n);
// stable sort of n records by 32-bit t; keys / vals: 2 * n uint32 each, tmp: n records
hipError_t dvs_sort(void *d_records, uint64_t n, int out_format, uint32_t *keys0, uint32_t *keys1, uint32_t *vals0,
                    uint32_t *vals1, void *tmp, void *temp, size_t temp_bytes, hipStream_t stream);
hipError_t dvs_log1p_run(const double *d_x, double *d_y, uint64_t n, hipStream_t stream);

}  // namespace adder
