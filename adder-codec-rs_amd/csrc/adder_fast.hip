// adder_fast.hip -- the dense FAST 9_16 detector and the confusion counts of include/adder_fast.h.
//   fast_score_kernel    one 128 x 32 tile per workgroup: the tile and its halo staged in LDS as bytes (one aligned
//                        global dword per lane, channel 0 picked while staging), four adjacent pixels per lane tested
//                        out of LDS, the mask / score bytes handed through LDS to stores of whole aligned dwords
//                        (bytes at the ends of a row segment) -- any width, any pointer alignment;
//   fast_nonmax_kernel   strict 3x3 suppression over the score plane;
//   fast_count_kernel    truth / predicted / both per frame: nonzero bytes of dwords, AND, popcount, wave reduction,
//                        one integer atomic per wave;
//   fast_scatter_kernel  the kept pixels to x | y << 16 behind hipcub's exclusive sum of the mask (the scan every
//                        event tool here uses);
//   fast_xy_*            a coordinate list back to a mask plane.
// The per-pixel rules are adder_fast_logic.hpp's.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include "adder_fast_kernels.h"
#include "adder_fast_logic.hpp"

namespace adder {

// FastPair on the device: (ring - c, c - ring) as the two 16-bit halves of one register, so that one packed min / max
// serves the bright and the dark direction
typedef short fast_short2 __attribute__((ext_vector_type(2)));
struct FastPairPk {
    fast_short2 v;
};
__device__ __forceinline__ FastPairPk fast_pair(int ring, int c, const FastPairPk *) {
    FastPairPk r;
    r.v.x = (short)(ring - c);
    r.v.y = (short)(c - ring);
    return r;
}
__device__ __forceinline__ FastPairPk fast_pmin(FastPairPk a, FastPairPk b) {
    return FastPairPk{__builtin_elementwise_min(a.v, b.v)};
}
__device__ __forceinline__ FastPairPk fast_pmax(FastPairPk a, FastPairPk b) {
    return FastPairPk{__builtin_elementwise_max(a.v, b.v)};
}
__device__ __forceinline__ int fast_phmax(FastPairPk a) { return a.v.x > a.v.y ? (int)a.v.x : (int)a.v.y; }

constexpr uint32_t kTileRows = kFastTileH + 2u * kFastHaloY;      // 38 staged rows
constexpr uint32_t kTilePitch = kFastTileW + 2u * kFastHaloX;     // 136 staged bytes per row
constexpr uint32_t kTilePitchDw = kTilePitch / 4u;
constexpr uint32_t kResPitchDw = kFastTileW / 4u;
constexpr uint32_t kStoreDw = kFastTileW / 4u + 1u;               // aligned dwords a row segment of the tile touches

// byte `col` of the three dwords a lane holds of one staged row
__device__ __forceinline__ int win_byte(const uint32_t (&row)[3], uint32_t col) {
    return (int)((row[col >> 2] >> (8u * (col & 3u))) & 0xffu);
}

// A row segment of the tile's result bytes (res: [kFastTileH][kFastTileW] in LDS) to plane memory at `a`, tw bytes:
// the aligned dwords inside the segment whole, the bytes in front of the first and behind the last one by one.
__device__ __forceinline__ void store_segment(const uint32_t *res_row, uintptr_t a, uint32_t tw, uint32_t j) {
    const uintptr_t q = (a & ~(uintptr_t)3) + 4u * j;
    if (q >= a + tw) return;
    if (q >= a && q + 4u <= a + tw) {
        const uint32_t off = (uint32_t)(q - a);
        const uint32_t lo = res_row[off >> 2];
        const uint32_t hi = (off & 3u) ? res_row[(off >> 2) + 1u] : 0u;
        *(uint32_t *)q = (uint32_t)((((uint64_t)hi << 32) | lo) >> (8u * (off & 3u)));
        return;
    }
    const uint8_t *rb = (const uint8_t *)res_row;
#pragma unroll
    for (uint32_t b = 0; b < 4; ++b) {
        const uintptr_t p = q + b;
        if (p >= a && p < a + tw) *(uint8_t *)p = rb[p - a];
    }
}

// frames / mask / score: the group's first frame.  mask or score may be null (not both).
template <uint32_t C>
__global__ __launch_bounds__(kFastBlock) void fast_score_kernel(const uint8_t *__restrict__ frames, uint32_t n_frames,
                                                                uint32_t w, uint32_t h, uint32_t tiles_x,
                                                                uint32_t tiles_y, int threshold, uint32_t want_score,
                                                                uint8_t *__restrict__ mask, uint8_t *__restrict__ score) {
    __shared__ uint32_t tile[kTileRows * kTilePitchDw];
    __shared__ uint32_t res_m[kFastTileH * kResPitchDw];
    __shared__ uint32_t res_s[kFastTileH * kResPitchDw];
    const uint32_t tid = threadIdx.x;
    const uint32_t tiles = tiles_x * tiles_y;
    const uint32_t f = blockIdx.x / tiles, t = blockIdx.x % tiles;
    const uint32_t tx = t % tiles_x, ty = t / tiles_x;
    const uint32_t x0 = tx * kFastTileW, y0 = ty * kFastTileH;
    const size_t frame_bytes = (size_t)w * h * C;
    const uintptr_t buf_lo = (uintptr_t)frames, buf_hi = buf_lo + (size_t)n_frames * frame_bytes;
    const uintptr_t fr = buf_lo + (size_t)f * frame_bytes;

    // ---- stage rows y0 - 3 .. y0 + 34, columns x0 - 4 .. x0 + 131, as far as they lie in the plane ----
    {
        constexpr uint32_t kRowDw = (kTilePitch * C + 6u) / 4u;  // aligned dwords over kTilePitch * C bytes at any phase
        const int xs = (int)x0 - (int)kFastHaloX, ys = (int)y0 - (int)kFastHaloY;
        const uint32_t xlo = xs < 0 ? 0u : (uint32_t)xs;
        const uint32_t xhi = (uint32_t)xs + kTilePitch < w ? (uint32_t)xs + kTilePitch : w;
        uint8_t *tb = (uint8_t *)tile;
        for (uint32_t i = tid; i < kTileRows * kRowDw; i += kFastBlock) {
            const uint32_t r = i / kRowDw, j = i % kRowDw;
            const int y = ys + (int)r;
            if (y < 0 || y >= (int)h) continue;
            const uintptr_t lo = fr + ((size_t)y * w + xlo) * C, hi = fr + ((size_t)y * w + xhi) * C;
            const uintptr_t q = (lo & ~(uintptr_t)3) + 4u * j;
            if (q >= hi) continue;
            uint32_t v = 0u;
            if (q >= buf_lo && q + 4u <= buf_hi) {
                v = *(const uint32_t *)q;
            } else {  // the first or the last dword of the whole input: only the bytes that belong to it
#pragma unroll
                for (uint32_t b = 0; b < 4; ++b)
                    if (q + b >= buf_lo && q + b < buf_hi) v |= (uint32_t)(*(const uint8_t *)(q + b)) << (8u * b);
            }
#pragma unroll
            for (uint32_t b = 0; b < 4; ++b) {
                const uintptr_t p = q + b;
                if (p < lo || p >= hi) continue;
                const uint32_t ro = (uint32_t)(p - lo);
                if (C != 1u && ro % C != 0u) continue;
                const uint32_t col = xlo - (uint32_t)xs + ro / C;  // xlo >= xs
                tb[r * kTilePitch + col] = (uint8_t)(v >> (8u * b));
            }
        }
    }
    __syncthreads();

    // ---- four adjacent pixels per lane, rows ly, ly + 8, ly + 16, ly + 24 of the tile ----
    const uint32_t lx = tid & 31u, ly = tid >> 5;
#pragma unroll 1
    for (uint32_t it = 0; it < kFastTileH / 8u; ++it) {
        const uint32_t row = ly + 8u * it;
        const uint32_t y = y0 + row, x = x0 + 4u * lx;
        uint32_t m = 0u, s = 0u;
        if (y < h && x < w) {
            uint32_t win[7][3];  // staged rows row .. row + 6 (the centre's is row + 3), staged bytes 4 lx .. 4 lx + 11
#pragma unroll
            for (uint32_t r = 0; r < 7; ++r)
#pragma unroll
                for (uint32_t d = 0; d < 3; ++d) win[r][d] = tile[(row + r) * kTilePitchDw + lx + d];
#pragma unroll
            for (uint32_t i = 0; i < 4; ++i) {
                if (!fast_candidate(w, h, x + i, y)) continue;
                const int c = win_byte(win[3], kFastHaloX + i);
                int ring[16];
#pragma unroll
                for (uint32_t k = 0; k < 16; ++k)
                    ring[k] = win_byte(win[3 + fast_ring_dy(k)], (uint32_t)((int)(kFastHaloX + i) + fast_ring_dx(k)));
                if (!fast_corner(c, ring, threshold)) continue;
                m |= 1u << (8u * i);
                if (want_score) s |= fast_score_byte<FastPairPk>(c, ring, threshold) << (8u * i);
            }
        }
        res_m[row * kResPitchDw + lx] = m;
        res_s[row * kResPitchDw + lx] = s;
    }
    __syncthreads();

    // ---- the tile's rows to the planes ----
    const uint32_t tw = w - x0 < kFastTileW ? w - x0 : kFastTileW;
    const uint32_t th = h - y0 < kFastTileH ? h - y0 : kFastTileH;
    for (uint32_t i = tid; i < kFastTileH * kStoreDw; i += kFastBlock) {
        const uint32_t row = i / kStoreDw, j = i % kStoreDw;
        if (row >= th) continue;
        const size_t at = ((size_t)f * h + (y0 + row)) * w + x0;
        if (mask) store_segment(res_m + row * kResPitchDw, (uintptr_t)mask + at, tw, j);
        if (score) store_segment(res_s + row * kResPitchDw, (uintptr_t)score + at, tw, j);
    }
}

// one lane: four adjacent pixels x = 4 g .. 4 g + 3 of one row; n_rows = frames * h
__global__ __launch_bounds__(kFastBlock) void fast_nonmax_kernel(const uint8_t *__restrict__ score, uint32_t n_rows,
                                                                 uint32_t w, uint32_t h, uint32_t quads,
                                                                 uint8_t *__restrict__ mask) {
    const uint32_t i = blockIdx.x * kFastBlock + threadIdx.x;
    if (i >= n_rows * quads) return;
    const uint32_t fy = i / quads, g = i % quads;
    const uint32_t y = fy % h, x = 4u * g;
    uint32_t v[3][6];  // rows y - 1 .. y + 1, columns x - 1 .. x + 4; outside the plane 0
#pragma unroll
    for (uint32_t r = 0; r < 3; ++r) {
        const int yy = (int)y + (int)r - 1;
        const bool row_in = yy >= 0 && yy < (int)h;
        const uint8_t *p = row_in ? score + ((size_t)fy + r - 1u) * w : score;  // (a frame's rows: fy = f * h + y)
        if (row_in && x + 4u <= w && (((uintptr_t)(p + x)) & 3u) == 0u) {
            const uint32_t d = *(const uint32_t *)(p + x);
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) v[r][1 + k] = (d >> (8u * k)) & 0xffu;
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) v[r][1 + k] = (row_in && x + k < w) ? p[x + k] : 0u;
        }
        v[r][0] = (row_in && x > 0u) ? p[x - 1u] : 0u;
        v[r][5] = (row_in && x + 4u < w) ? p[x + 4u] : 0u;
    }
    uint32_t m = 0u;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t nb[8] = {v[0][k], v[0][k + 1], v[0][k + 2], v[1][k], v[1][k + 2], v[2][k], v[2][k + 1], v[2][k + 2]};
        m |= (fast_nonmax_keep(v[1][k + 1], nb) ? 1u : 0u) << (8u * k);
    }
    uint8_t *o = mask + (size_t)fy * w + x;
    if (x + 4u <= w && (((uintptr_t)o) & 3u) == 0u) {
        *(uint32_t *)o = m;
    } else {
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k)
            if (x + k < w) o[k] = (uint8_t)(m >> (8u * k));
    }
}

// grid (blocks, frames of the group); a lane walks groups of four positions of its frame
__global__ __launch_bounds__(kFastBlock) void fast_count_kernel(const uint8_t *__restrict__ mask,
                                                                const uint8_t *__restrict__ pred, uint64_t plane,
                                                                FastFrameSums *__restrict__ sums) {
    const uint32_t f = blockIdx.y;
    const uint8_t *mf = mask + (size_t)f * plane;
    const uint8_t *pf = pred ? pred + (size_t)f * plane : nullptr;
    uint32_t gt = 0u, pr = 0u, both = 0u;  // a plane has fewer than 2^31 positions
    const uint64_t step = 4ull * kFastBlock * gridDim.x;
    for (uint64_t i = 4ull * (blockIdx.x * kFastBlock + threadIdx.x); i < plane; i += step) {
        uint32_t a = 0u, b = 0u;
        const bool whole = i + 4u <= plane;
        if (whole && (((uintptr_t)(mf + i)) & 3u) == 0u) {
            a = *(const uint32_t *)(mf + i);
        } else {
            for (uint32_t k = 0; k < 4 && i + k < plane; ++k) a |= (uint32_t)mf[i + k] << (8u * k);
        }
        if (pf) {
            if (whole && (((uintptr_t)(pf + i)) & 3u) == 0u) {
                b = *(const uint32_t *)(pf + i);
            } else {
                for (uint32_t k = 0; k < 4 && i + k < plane; ++k) b |= (uint32_t)pf[i + k] << (8u * k);
            }
        }
        a = fast_nonzero_bytes(a);
        b = fast_nonzero_bytes(b);
        gt += (uint32_t)__popc(a);
        pr += (uint32_t)__popc(b);
        both += (uint32_t)__popc(a & b);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        gt += __shfl_down(gt, d, 64);
        pr += __shfl_down(pr, d, 64);
        both += __shfl_down(both, d, 64);
    }
    if ((threadIdx.x & 63u) == 0u) {
        if (gt) atomicAdd(&sums[f].gt, (unsigned long long)gt);
        if (pr) atomicAdd(&sums[f].pred, (unsigned long long)pr);
        if (both) atomicAdd(&sums[f].both, (unsigned long long)both);
    }
}

struct FastFlag {
    __host__ __device__ __forceinline__ uint32_t operator()(const uint8_t &m) const { return m ? 1u : 0u; }
};

// mask / offs: the group's n positions; base: kept pixels of the frames in front of the group
__global__ __launch_bounds__(kFastBlock) void fast_scatter_kernel(const uint8_t *__restrict__ mask,
                                                                  const uint32_t *__restrict__ offs, uint32_t n,
                                                                  uint32_t w, uint32_t plane, uint64_t base,
                                                                  uint32_t *__restrict__ xy, uint64_t cap) {
    const uint32_t i = blockIdx.x * kFastBlock + threadIdx.x;
    if (i >= n || !mask[i]) return;
    const uint32_t r = i % plane;
    const uint64_t o = base + offs[i];
    if (o < cap) xy[o] = (r % w) | ((r / w) << 16);
}

__global__ __launch_bounds__(kFastBlock) void fast_xy_check_kernel(const uint32_t *__restrict__ xy, uint64_t n,
                                                                   uint32_t w, uint32_t h, uint32_t *__restrict__ bad) {
    const uint64_t i = (uint64_t)blockIdx.x * kFastBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t v = xy[i];
    if ((v & 0xffffu) >= w || (v >> 16) >= h) atomicOr(bad, 1u);
}

__global__ __launch_bounds__(kFastBlock) void fast_xy_mask_kernel(const uint32_t *__restrict__ xy, uint64_t n,
                                                                  uint32_t w, uint32_t h, uint8_t *__restrict__ mask) {
    const uint64_t i = (uint64_t)blockIdx.x * kFastBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t v = xy[i], x = v & 0xffffu, y = v >> 16;
    if (x < w && y < h) mask[(size_t)y * w + x] = 1u;
}

FastShape fast_shape(uint32_t width, uint32_t height, uint32_t channels) {
    FastShape s{};
    s.width = width;
    s.height = height;
    s.channels = channels;
    s.tiles_x = (width + kFastTileW - 1u) / kFastTileW;
    s.tiles_y = (height + kFastTileH - 1u) / kFastTileH;
    s.plane = (uint64_t)width * height;
    s.frame_bytes = s.plane * channels;
    return s;
}

uint32_t fast_group_frames(const FastShape &s) {
    const uint64_t g = (uint64_t)INT32_MAX / s.plane;  // the plane itself is below 2^31 (adder_fast_create)
    return (uint32_t)(g < 1u ? 1u : g > 65535u ? 65535u : g);
}

size_t fast_scan_temp_bytes(const FastShape &s, uint32_t n) {
    const uint32_t g = fast_group_frames(s);
    const uint64_t elems = (uint64_t)(n < g ? n : g) * s.plane;
    size_t b = 0;
    hipcub::TransformInputIterator<uint32_t, FastFlag, const uint8_t *> it(nullptr, FastFlag());
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, b, it, (uint32_t *)nullptr, (int)elems);
    return b + 256;
}

hipError_t fast_detect_run(const FastShape &s, const uint8_t *d_frames, uint32_t n, int threshold, bool nonmax,
                           uint8_t *d_mask, uint8_t *d_score, hipStream_t stream) {
    const uint32_t group = fast_group_frames(s), tiles = s.tiles_x * s.tiles_y;
    const uint32_t quads = (s.width + 3u) / 4u;
    for (uint32_t f0 = 0; f0 < n; f0 += group) {
        const uint32_t nf = n - f0 < group ? n - f0 : group;
        const uint8_t *fr = d_frames + (size_t)f0 * s.frame_bytes;
        uint8_t *mk = d_mask + (size_t)f0 * s.plane;
        uint8_t *sc = d_score ? d_score + (size_t)f0 * s.plane : nullptr;
        uint8_t *score_mask = nonmax ? nullptr : mk;  // with nonmax the mask comes from the suppression
        const uint32_t want_score = sc ? 1u : 0u;
        if (s.channels == 1u)
            hipLaunchKernelGGL(fast_score_kernel<1u>, dim3(tiles * nf), dim3(kFastBlock), 0, stream, fr, nf, s.width,
                               s.height, s.tiles_x, s.tiles_y, threshold, want_score, score_mask, sc);
        else
            hipLaunchKernelGGL(fast_score_kernel<3u>, dim3(tiles * nf), dim3(kFastBlock), 0, stream, fr, nf, s.width,
                               s.height, s.tiles_x, s.tiles_y, threshold, want_score, score_mask, sc);
        if (nonmax) {
            const uint32_t rows = nf * s.height;
            const uint32_t grid = (uint32_t)(((uint64_t)rows * quads + kFastBlock - 1u) / kFastBlock);
            hipLaunchKernelGGL(fast_nonmax_kernel, dim3(grid), dim3(kFastBlock), 0, stream, sc, rows, s.width, s.height,
                               quads, mk);
        }
    }
    return hipGetLastError();
}

hipError_t fast_count_run(const FastShape &s, const uint8_t *d_mask, const uint8_t *d_pred, uint32_t n,
                          FastFrameSums *d_sums, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(d_sums, 0, (size_t)n * sizeof(FastFrameSums), stream);
    if (e != hipSuccess) return e;
    const uint64_t per_block = 4ull * kFastBlock;
    uint64_t blocks = (s.plane + per_block - 1u) / per_block;
    if (blocks > kFastCountBlocks) blocks = kFastCountBlocks;
    for (uint32_t f0 = 0; f0 < n; f0 += 65535u) {
        const uint32_t nf = n - f0 < 65535u ? n - f0 : 65535u;
        hipLaunchKernelGGL(fast_count_kernel, dim3((uint32_t)blocks, nf), dim3(kFastBlock), 0, stream,
                           d_mask + (size_t)f0 * s.plane, d_pred ? d_pred + (size_t)f0 * s.plane : nullptr, s.plane,
                           d_sums + f0);
    }
    return hipGetLastError();
}

hipError_t fast_compact_run(const FastShape &s, const uint8_t *d_mask, uint32_t n, const uint64_t *counts,
                            uint32_t *offs, void *temp, size_t temp_bytes, uint32_t *d_xy, uint64_t cap,
                            hipStream_t stream) {
    const uint32_t group = fast_group_frames(s);
    uint64_t base = 0;
    for (uint32_t f0 = 0; f0 < n; f0 += group) {
        const uint32_t nf = n - f0 < group ? n - f0 : group;
        const uint32_t elems = (uint32_t)(nf * s.plane);  // below 2^31
        const uint8_t *mk = d_mask + (size_t)f0 * s.plane;
        hipcub::TransformInputIterator<uint32_t, FastFlag, const uint8_t *> flags(mk, FastFlag());
        size_t tb = temp_bytes;
        const hipError_t e = hipcub::DeviceScan::ExclusiveSum(temp, tb, flags, offs, (int)elems, stream);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(fast_scatter_kernel, dim3((elems + kFastBlock - 1u) / kFastBlock), dim3(kFastBlock), 0, stream,
                           mk, offs, elems, s.width, (uint32_t)s.plane, base, d_xy, cap);
        for (uint32_t k = 0; k < nf; ++k) base += counts[f0 + k];
    }
    return hipGetLastError();
}

hipError_t fast_xy_check_run(const FastShape &s, const uint32_t *d_xy, uint64_t n, uint32_t *d_bad, hipStream_t stream) {
    if (n == 0u) return hipSuccess;
    hipLaunchKernelGGL(fast_xy_check_kernel, dim3((uint32_t)((n + kFastBlock - 1u) / kFastBlock)), dim3(kFastBlock), 0,
                       stream, d_xy, n, s.width, s.height, d_bad);
    return hipGetLastError();
}

hipError_t fast_xy_mask_run(const FastShape &s, const uint32_t *d_xy, uint64_t n, uint8_t *d_mask, hipStream_t stream) {
    const hipError_t e = hipMemsetAsync(d_mask, 0, (size_t)s.plane, stream);
    if (e != hipSuccess || n == 0u) return e;
    hipLaunchKernelGGL(fast_xy_mask_kernel, dim3((uint32_t)((n + kFastBlock - 1u) / kFastBlock)), dim3(kFastBlock), 0,
                       stream, d_xy, n, s.width, s.height, d_mask);
    return hipGetLastError();
}

}  // namespace adder
