// adder_quality.hip -- MSE and SSIM of reconstructed frames (include/adder_quality.h; cv.rs:306-430).
//
// Two batches of n u8 frames [n][H][W][C], C interleaved.
//   1. SSE: a grid-stride sum of (a - b)^2 per frame, u64 partials per block.  Integer and exact: any order gives the
//      host mirror's value.
//   2. SSIM (only when asked): a block owns a tile of 248 x 32 windows of one (frame, channel).  Thread t owns pixel
//      column x0 + t and slides its integer vertical 8-sums of x, y, x*y, x^2, y^2 down the tile, the last eight
//      rows' pixels in registers; each row step publishes the sums in LDS and the threads of the window columns add
//      eight neighbours.  From the five integer box sums every intermediate of cv.rs's mean / variance / covariance
//      is exact, so only the reference's last f64 operations round, in its order: the window's value is
//      the reference's bit for bit.  A thread sums 64 * r over its windows in row order, the block in a fixed tree.
//   3. combine: a block per frame adds the SSE partials and each channel's tile partials in a fixed order.
// Nothing uses float atomics: a frame's numbers do not depend on the run or on the other frames of the call.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "adder_quality_kernels.h"

namespace adder {

__device__ __forceinline__ uint32_t sq_bytes(uint32_t x, uint32_t y) {
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < 32; k += 8) {
        const int d = (int)((x >> k) & 0xffu) - (int)((y >> k) & 0xffu);
        s += (uint32_t)(d * d);
    }
    return s;
}

// fixed-order block sums (a tree over the wave, then the four waves in order); the result is valid in thread 0
__device__ __forceinline__ unsigned long long block_sum_u64(unsigned long long v, unsigned long long *sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63u) == 0u) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return sh[0] + sh[1] + sh[2] + sh[3];
}

__device__ __forceinline__ double block_sum_f64(double v, double *sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63u) == 0u) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// grid (sse_blocks, frames of the group); VEC: frames and pointers 16-byte aligned
template <bool VEC>
__global__ __launch_bounds__(kQualBlock) void quality_sse_kernel(const uint8_t *__restrict__ a,
                                                                const uint8_t *__restrict__ b, uint64_t frame_bytes,
                                                                uint32_t f0, unsigned long long *__restrict__ part) {
    __shared__ unsigned long long sh[4];
    const uint64_t f = f0 + blockIdx.y;
    const uint8_t *fa = a + f * frame_bytes, *fb = b + f * frame_bytes;
    const uint64_t stride = (uint64_t)gridDim.x * kQualBlock;
    unsigned long long acc = 0;
    if (VEC) {
        const uint4 *va = reinterpret_cast<const uint4 *>(fa), *vb = reinterpret_cast<const uint4 *>(fb);
        const uint64_t n16 = frame_bytes / 16u;
        for (uint64_t i = (uint64_t)blockIdx.x * kQualBlock + threadIdx.x; i < n16; i += stride) {
            const uint4 x = va[i], y = vb[i];
            acc += sq_bytes(x.x, y.x) + sq_bytes(x.y, y.y) + sq_bytes(x.z, y.z) + sq_bytes(x.w, y.w);
        }
    } else {
        for (uint64_t i = (uint64_t)blockIdx.x * kQualBlock + threadIdx.x; i < frame_bytes; i += stride) {
            const int d = (int)fa[i] - (int)fb[i];
            acc += (unsigned long long)(d * d);
        }
    }
    const unsigned long long s = block_sum_u64(acc, sh);
    if (threadIdx.x == 0) part[f * gridDim.x + blockIdx.x] = s;
}

// grid (tiles_x * tiles_y, frames of the group * channels)
__global__ __launch_bounds__(kQualBlock) void quality_ssim_kernel(const uint8_t *__restrict__ a,
                                                                 const uint8_t *__restrict__ b, QualityShape s,
                                                                 uint32_t f0, double *__restrict__ map,
                                                                 double *__restrict__ part) {
    __shared__ uint4 col[2][kQualBlock];  // per pixel column: {sum x | sum y << 16, sum xy, sum x^2, sum y^2}
    __shared__ double sh[4];
    const uint32_t C = s.channels, W = s.width;
    const uint32_t ww = s.width - 7u, wh = s.height - 7u;  // windows per row, per column
    const uint32_t tiles = s.tiles_x * s.tiles_y;
    const uint32_t tile = blockIdx.x, ch = blockIdx.y % C;
    const uint64_t f = f0 + blockIdx.y / C;
    const uint32_t x0 = (tile % s.tiles_x) * kSsimTileW, y0 = (tile / s.tiles_x) * kSsimTileH;
    const uint32_t rows = min(kSsimTileH, wh - y0);  // window rows of this tile (block-uniform)
    const uint32_t t = threadIdx.x;
    const bool col_ok = t < kSsimTileW + 7u && x0 + t < W;  // this thread's pixel column exists
    const bool win_ok = t < kSsimTileW && x0 + t < ww;       // ... and a window starts on it
    const uint64_t rstride = (uint64_t)W * C;
    const uint64_t base = f * s.frame_bytes + (uint64_t)y0 * rstride + (uint64_t)(x0 + t) * C + ch;
    const uint8_t *pa = a + (col_ok ? base : 0u), *pb = b + (col_ok ? base : 0u);

    // the column's last eight pixel rows, and their sums
    uint32_t ra[8], rb[8];
    uint32_t vx = 0, vy = 0, vxy = 0, vxx = 0, vyy = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        ra[i] = col_ok ? pa[(uint64_t)i * rstride] : 0u;
        rb[i] = col_ok ? pb[(uint64_t)i * rstride] : 0u;
        vx += ra[i];
        vy += rb[i];
        vxy += ra[i] * rb[i];
        vxx += ra[i] * ra[i];
        vyy += rb[i] * rb[i];
    }
    double acc = 0.0;
    double *mrow = map ? map + ((f * C + ch) * wh + y0) * (uint64_t)ww + x0 + t : nullptr;
    for (uint32_t k0 = 0; k0 < rows; k0 += 8u) {
#pragma unroll
        for (uint32_t j = 0; j < 8u; ++j) {
            const uint32_t k = k0 + j;
            if (k >= rows) break;
            const bool more = k + 1u < rows;
            uint32_t na = 0u, nb = 0u;  // the pixel row entering after this step: y0 + k + 8
            if (more && col_ok) {
                na = pa[(uint64_t)(k + 8u) * rstride];
                nb = pb[(uint64_t)(k + 8u) * rstride];
            }
            col[j & 1u][t] = make_uint4(vx | (vy << 16), vxy, vxx, vyy);  // (8 * 255 < 2^16: no carry into y)
            __syncthreads();  // (two buffers: the step before last read the other one before this barrier)
            if (win_ok) {
                uint32_t P = 0u, sxy = 0u, sxx = 0u, syy = 0u;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const uint4 v = col[j & 1u][t + i];
                    P += v.x;  // (64 * 255 < 2^16: the packed halves stay apart)
                    sxy += v.y;
                    sxx += v.z;
                    syy += v.w;
                }
                const int sx = (int)(P & 0xffffu), sy = (int)(P >> 16);
                // cv.rs:398-407 on exact values: 2 mx my, 2 cov, mx^2 + my^2, vx + vy (every integer below 2^31)
                const double m2 = (double)(2 * sx * sy) / 4096.0;
                const double cv2 = (double)(64 * (int)sxy - sx * sy) / 32.0;
                const double mm = (double)(sx * sx + sy * sy) / 4096.0;
                const double vv = (double)(64 * (int)sxx - sx * sx + 64 * (int)syy - sy * sy) / 64.0;
                const double counter = (m2 + kSsimC1) * (cv2 + kSsimC2);
                const double denominator = (mm + kSsimC1) * (vv + kSsimC2);
                const double r = counter / denominator;
                acc += r * 64.0;
                if (mrow) mrow[(uint64_t)k * ww] = r;
            }
            if (more) {
                vx += na - ra[j];
                vy += nb - rb[j];
                vxy += na * nb - ra[j] * rb[j];
                vxx += na * na - ra[j] * ra[j];
                vyy += nb * nb - rb[j] * rb[j];
                ra[j] = na;
                rb[j] = nb;
            }
        }
    }
    const double sum = block_sum_f64(acc, sh);
    if (t == 0) part[(f * C + ch) * tiles + tile] = sum;
}

// grid (frames of the group): the fixed-order combine of a frame's partials
__global__ __launch_bounds__(kQualBlock) void quality_sums_kernel(const unsigned long long *__restrict__ sse_part,
                                                                 const double *__restrict__ ssim_part, QualityShape s,
                                                                 uint32_t f0, QualityFrameSums *__restrict__ out) {
    __shared__ unsigned long long shu[4];
    __shared__ double shd[3][4];
    const uint64_t f = f0 + blockIdx.x;
    const uint32_t t = threadIdx.x;
    unsigned long long u = 0;
    for (uint32_t i = t; i < s.sse_blocks; i += kQualBlock) u += sse_part[f * s.sse_blocks + i];
    const unsigned long long sse = block_sum_u64(u, shu);
    double d[3] = {0.0, 0.0, 0.0};
    if (ssim_part) {
        const uint32_t tiles = s.tiles_x * s.tiles_y;
        for (uint32_t ch = 0; ch < s.channels; ++ch) {
            double v = 0.0;
            for (uint32_t i = t; i < tiles; i += kQualBlock) v += ssim_part[(f * s.channels + ch) * tiles + i];
            d[ch] = block_sum_f64(v, shd[ch]);
        }
    }
    if (t == 0) {
        QualityFrameSums r;
        r.sse = sse;
        r.ssim64[0] = d[0];
        r.ssim64[1] = d[1];
        r.ssim64[2] = d[2];
        out[f] = r;
    }
}

QualityShape quality_shape(uint32_t width, uint32_t height, uint32_t channels) {
    QualityShape s{};
    s.width = width;
    s.height = height;
    s.channels = channels;
    s.frame_bytes = (uint64_t)width * height * channels;
    if (width >= 8u && height >= 8u) {
        s.tiles_x = (width - 7u + kSsimTileW - 1u) / kSsimTileW;
        s.tiles_y = (height - 7u + kSsimTileH - 1u) / kSsimTileH;
        s.windows = (uint64_t)(width - 7u) * (height - 7u);
    }
    const uint64_t nb = (s.frame_bytes + kSseBytesPerBlock - 1u) / kSseBytesPerBlock;
    s.sse_blocks = (uint32_t)(nb < 1u ? 1u : nb > kSseMaxBlocks ? kSseMaxBlocks : nb);
    return s;
}

uint32_t quality_group_frames(const QualityShape &s) {
    const uint64_t limit = 0xffffffffull / kQualBlock;  // blocks of one launch
    const uint64_t per_frame_ssim = (uint64_t)s.tiles_x * s.tiles_y * s.channels;
    uint64_t g = 65535u / s.channels;
    if (per_frame_ssim && limit / per_frame_ssim < g) g = limit / per_frame_ssim;
    if (limit / s.sse_blocks < g) g = limit / s.sse_blocks;
    return (uint32_t)(g < 1u ? 1u : g);
}

hipError_t quality_run(const QualityShape &s, const uint8_t *d_a, const uint8_t *d_b, uint32_t n, bool ssim,
                       double *d_map, unsigned long long *sse_part, double *ssim_part, QualityFrameSums *d_sums,
                       hipStream_t stream) {
    const bool vec = ((uintptr_t)d_a % 16u) == 0u && ((uintptr_t)d_b % 16u) == 0u && s.frame_bytes % 16u == 0u;
    const bool run_ssim = ssim && s.windows != 0u;
    const uint32_t group = quality_group_frames(s);
    for (uint32_t f0 = 0; f0 < n; f0 += group) {
        const uint32_t g = n - f0 < group ? n - f0 : group;
        if (vec)
            hipLaunchKernelGGL(quality_sse_kernel<true>, dim3(s.sse_blocks, g), dim3(kQualBlock), 0, stream, d_a, d_b,
                               s.frame_bytes, f0, sse_part);
        else
            hipLaunchKernelGGL(quality_sse_kernel<false>, dim3(s.sse_blocks, g), dim3(kQualBlock), 0, stream, d_a, d_b,
                               s.frame_bytes, f0, sse_part);
        if (run_ssim)
            hipLaunchKernelGGL(quality_ssim_kernel, dim3(s.tiles_x * s.tiles_y, g * s.channels), dim3(kQualBlock), 0,
                               stream, d_a, d_b, s, f0, d_map, ssim_part);
        hipLaunchKernelGGL(quality_sums_kernel, dim3(g), dim3(kQualBlock), 0, stream, sse_part,
                           run_ssim ? ssim_part : nullptr, s, f0, d_sums);
    }
    return hipGetLastError();
}

}  // namespace adder
