// adder_chain.hip -- what the Prophesee and the DAVIS source do alike between their own kernels (adder_chain_kernels.h):
// a stable radix sort of (key, index) pairs, the exclusive scan of the records' step counts with its total, and the
// compaction of the records' two step slots.  The one place that instantiates hipcub for the two sources.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include "adder_chain_kernels.h"

namespace adder {

__global__ void chain_total_kernel(const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ offs, uint64_t n,
                                   unsigned long long *total) {
    *total = (unsigned long long)offs[n - 1] + cnt[n - 1];
}

__global__ __launch_bounds__(256) void chain_scatter_kernel(uint64_t n, const uint32_t *__restrict__ cnt,
                                                            const uint32_t *__restrict__ offs,
                                                            const AdderSparseStep *__restrict__ stage,
                                                            AdderSparseStep *__restrict__ steps) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = cnt[i];
    const uint64_t o = offs[i];
    for (uint32_t k = 0; k < c; ++k) steps[o + k] = stage[2u * i + k];
}

size_t chain_temp_bytes(uint64_t n_records, uint32_t n_plane) {
    size_t a = 0, b = 0, c = 0;
    if (n_records) {
        hipcub::DoubleBuffer<uint32_t> k(nullptr, nullptr), v(nullptr, nullptr);
        (void)hipcub::DeviceRadixSort::SortPairs(nullptr, a, k, v, (int)n_records);
        (void)hipcub::DeviceScan::ExclusiveSum(nullptr, b, (const uint32_t *)nullptr, (uint32_t *)nullptr, (int)n_records);
    }
    if (n_plane)
        (void)hipcub::DeviceScan::ExclusiveSum(nullptr, c, (const uint32_t *)nullptr, (uint32_t *)nullptr, (int)n_plane);
    if (b > a) a = b;
    if (c > a) a = c;
    return a + 256;
}

hipError_t chain_sort_pairs(const ChainScratch &s, uint64_t n, int bits, hipStream_t stream) {
    size_t temp_bytes = s.temp_bytes;  // hipcub takes it by reference
    hipcub::DoubleBuffer<uint32_t> k(s.keys0, s.keys1), v(s.idx0, s.idx1);
    hipError_t e = hipcub::DeviceRadixSort::SortPairs(s.temp, temp_bytes, k, v, (int)n, 0, bits, stream);
    if (e != hipSuccess) return e;
    // an odd number of radix passes leaves the result in the second buffers
    if (k.Current() != s.keys0) {
        e = hipMemcpyAsync(s.keys0, k.Current(), n * 4u, hipMemcpyDeviceToDevice, stream);
        if (e != hipSuccess) return e;
    }
    if (v.Current() != s.idx0) e = hipMemcpyAsync(s.idx0, v.Current(), n * 4u, hipMemcpyDeviceToDevice, stream);
    return e;
}

hipError_t chain_exclusive_sum(const ChainScratch &s, const uint32_t *cnt, uint32_t *offs, uint64_t n,
                               hipStream_t stream) {
    size_t temp_bytes = s.temp_bytes;
    return hipcub::DeviceScan::ExclusiveSum(s.temp, temp_bytes, cnt, offs, (int)n, stream);
}

hipError_t chain_scan_counts(const ChainScratch &s, uint64_t n, unsigned long long *total_dst, hipStream_t stream) {
    const hipError_t e = chain_exclusive_sum(s, s.cnt, s.offs, n, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(chain_total_kernel, dim3(1), dim3(1), 0, stream, s.cnt, s.offs, n, total_dst);
    return hipGetLastError();
}

hipError_t chain_scatter(const ChainScratch &s, uint64_t n, AdderSparseStep *d_steps, hipStream_t stream) {
    hipLaunchKernelGGL(chain_scatter_kernel, dim3(grid_of(n)), dim3(256), 0, stream, n, s.cnt, s.offs, s.stage, d_steps);
    return hipGetLastError();
}

}  // namespace adder
