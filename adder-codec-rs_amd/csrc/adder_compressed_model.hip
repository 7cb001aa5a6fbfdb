// adder_compressed_model.hip -- the compressed codec's source model on the device: everything
// compress_adu does in front of the range coder, over events in HBM.  gfx950, wave64.
//
//   cut     the ADU of every event.  The rule is a serial recurrence (an event with t > start_t + span closes the ADU
//           and advances start_t), but cuts are rare: a parallel pass takes the maximum t of every 64 events, one
//           wave walks those maxima 64 at a time and only resolves the chunks that can trigger, with ballots
//           (cm_cut_block), and a parallel pass gives every event its number from its chunk's start state.
//   group   key = (ADU, cube, pixel), a stable radix sort of (key, index), run starts by flag + scan.  The sorted
//           order is the coder's order (cubes row-major; c, y, x) and the decoder's digest order at once.
//   model   a lane per non-empty pixel of an ADU: the intra symbols of its first event against the previous run's
//           first event (the previous non-empty pixel of the cube IS the previous run), then the drop rule and the
//           inter walk over its list (adder_compressed_logic.hpp).  Run twice: counting, then -- after the scans
//           have placed every pixel -- writing.  Empty pixels, skipped cubes, start_t and eof are filled by their
//           own kernels, each position from the same sums.
// No atomics: every store goes to a position a scan assigned.  All stores are ordinary vector stores.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include "adder_compressed_kernels.h"
#include "adder_sort_util.hpp"

namespace adder {

namespace {

__device__ __forceinline__ uint64_t cm_lower_bound(const uint64_t *__restrict__ keys, uint64_t lo, uint64_t hi,
                                                   uint64_t want) {  // first j in [lo, hi) with keys[j] >= want, or hi
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2u;
        if (keys[mid] < want)
            lo = mid + 1u;
        else
            hi = mid;
    }
    return lo;
}

// ---------------------------------------------------------------- cut
__global__ __launch_bounds__(256) void cm_chunk_kernel(const AdderEvent *__restrict__ ev, uint64_t n, uint32_t width,
                                                       uint32_t height, uint32_t channels, uint32_t *__restrict__ bmax,
                                                       uint32_t *__restrict__ bbad) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t t = 0;
    bool bad = false;
    if (i < n) {
        const AdderEvent e = ev[i];
        t = e.t;
        const uint32_t c = e.c == ADDER_C_NONE ? 0u : e.c;
        bad = e.x >= width || e.y >= height || c >= channels;
    }
    for (int o = 32; o; o >>= 1) {
        const uint32_t v = __shfl_xor(t, o);
        t = v > t ? v : t;
    }
    const uint64_t b = __ballot(bad);
    const uint64_t chunk = i >> 6;
    if (lane == 0u && chunk * kCmChunk < n) {
        bmax[chunk] = t;
        bbad[chunk] = b ? 1u : 0u;
    }
}

// one wave; chunk c's state before its first event goes to cstart[c] / cadu[c]
__global__ __launch_bounds__(64) void cm_walk_kernel(const AdderEvent *__restrict__ ev, uint64_t n, uint64_t nchunks,
                                                     const uint32_t *__restrict__ bmax,
                                                     const uint32_t *__restrict__ bbad, uint32_t start_t, uint32_t span,
                                                     uint32_t *__restrict__ cstart, uint32_t *__restrict__ cadu,
                                                     CmCutResult *res) {
    const uint32_t lane = threadIdx.x;
    uint32_t k = 0, bad = 0;
    for (uint64_t g = 0; g < nchunks; g += 64u) {
        const uint64_t ch = g + lane;
        const bool in = ch < nchunks;
        const uint32_t bm = in ? bmax[ch] : 0u;
        if (in) bad |= bbad[ch];
        uint64_t open = ~0ull;  // the group's chunks not yet passed
        while (open) {          // wave-uniform
            const uint64_t m = __ballot(in && bm > (uint32_t)(start_t + span)) & open;
            const uint32_t f = m ? (uint32_t)__builtin_ctzll(m) : 64u;
            if (in && ((open >> lane) & 1ull) && lane <= f) {  // up to and including the chunk that triggers
                cstart[ch] = start_t;
                cadu[ch] = k;
            }
            if (f == 64u) break;
            const uint64_t i = (g + f) * kCmChunk + lane;
            const bool valid = i < n;
            const uint32_t t = valid ? ev[i].t : 0u;
            const uint64_t cuts = cm_cut_block([&](uint32_t thr) { return (uint64_t)__ballot(valid && t > thr); }, &start_t, span);
            k += cm_popcount64(cuts);
            open = f == 63u ? 0ull : ~0ull << (f + 1u);
        }
    }
    const uint64_t any_bad = __ballot(bad != 0u);
    if (lane == 0u) {
        res->k = k;
        res->start_t = start_t;
        res->bad = any_bad ? 1u : 0u;
        res->pad = 0u;
        res->p_new = n;
    }
}

__global__ __launch_bounds__(256) void cm_number_kernel(const AdderEvent *__restrict__ ev, uint64_t n, uint32_t span,
                                                        const uint32_t *__restrict__ bmax,
                                                        const uint32_t *__restrict__ cstart,
                                                        const uint32_t *__restrict__ cadu, uint32_t *__restrict__ adu,
                                                        CmCutResult *res) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t chunk = i >> 6;
    if (chunk * kCmChunk >= n) return;  // the whole wave
    const bool valid = i < n;
    const uint32_t t = valid ? ev[i].t : 0u;
    uint32_t start_t = cstart[chunk];
    const uint32_t base = cadu[chunk];
    uint64_t cuts = 0;
    if (bmax[chunk] > (uint32_t)(start_t + span))  // wave-uniform
        cuts = cm_cut_block([&](uint32_t thr) { return (uint64_t)__ballot(valid && t > thr); }, &start_t, span);
    if (!valid) return;
    const uint32_t a = base + cm_cuts_upto(cuts, lane);
    const uint32_t before = lane ? base + cm_cuts_upto(cuts, lane - 1u) : base;
    adu[i] = a;
    const uint32_t k = res->k;
    if (a == k && before < k) res->p_new = i;  // one event at most
}

// ---------------------------------------------------------------- group
__global__ __launch_bounds__(256) void cm_keys_kernel(const AdderEvent *__restrict__ work, uint64_t carry, uint64_t p,
                                                      const uint32_t *__restrict__ adu, CmShape sh,
                                                      uint64_t *__restrict__ keys, uint32_t *__restrict__ vals) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= p) return;
    const AdderEvent e = work[i];
    const uint64_t a = i < carry ? 0u : adu[i - carry];
    keys[i] = cm_key(a, sh.ncubes, sh.bx, e.x, e.y, e.c == ADDER_C_NONE ? 0u : e.c);
    vals[i] = (uint32_t)i;
}

__global__ __launch_bounds__(256) void cm_heads_kernel(const AdderEvent *__restrict__ work,
                                                       const uint64_t *__restrict__ keys,
                                                       const uint32_t *__restrict__ vals, uint64_t p,
                                                       uint8_t *__restrict__ sd, uint32_t *__restrict__ st,
                                                       uint32_t *__restrict__ phead, uint32_t *__restrict__ chead) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j > p) return;
    if (j == p) {  // the sentinel: the scans' last entry is the number of runs
        phead[j] = 0u;
        chead[j] = 0u;
        return;
    }
    const AdderEvent e = work[vals[j]];
    sd[j] = e.d;
    st[j] = e.t;
    const uint64_t key = keys[j];
    const uint64_t prev = j ? keys[j - 1u] : ~0ull;
    phead[j] = j == 0u || prev != key ? 1u : 0u;
    chead[j] = j == 0u || (prev >> kCmPixBits) != (key >> kCmPixBits) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void cm_runs_kernel(uint64_t p, CmScratch s) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j > p) return;
    if (j == p) {
        s.prun_ev[s.pscan[p]] = (uint32_t)p;
        s.crun_ev[s.cscan[p]] = (uint32_t)p;
        s.res->runs_pixel = s.pscan[p];
        s.res->runs_cube = s.cscan[p];
        return;
    }
    if (s.phead[j]) s.prun_ev[s.pscan[j]] = (uint32_t)j;
    if (s.chead[j]) s.crun_ev[s.cscan[j]] = (uint32_t)j;
}

// ---------------------------------------------------------------- model
struct CmNoNote {
    __device__ void operator()(uint64_t, uint32_t, uint32_t) const {}
};

// where ADU a's symbols begin, its intra part's size, and the sums its runs subtract
struct CmAduBase {
    uint64_t sym, intra, sx0, si0;
    uint32_t crun0;
};
__device__ __forceinline__ CmAduBase cm_adu_base(const CmShape &sh, const CmScratch &s, uint64_t a) {
    CmAduBase b;
    const uint32_t r0 = s.adu_prun[a], r1 = s.adu_prun[a + 1u];
    b.crun0 = s.adu_crun[a];
    b.sx0 = s.sx[r0];
    b.si0 = s.si[r0];
    b.sym = s.adu_sym_off[a] + 4u;
    b.intra = cm_adu_intra_symbols(sh.ncubes, sh.npix, s.adu_crun[a + 1u] - b.crun0, s.sx[r1] - b.sx0);
    return b;
}

template <bool WRITE>
__global__ __launch_bounds__(256) void cm_model_kernel(CmShape sh, const uint64_t *__restrict__ keys, uint64_t p,
                                                       uint64_t runs, uint32_t start0, CmScratch s,
                                                       uint16_t *__restrict__ sym) {
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (!WRITE && r == runs) {  // the sentinels of the scans over runs and over kept flags
        s.intra_extra[r] = 0u;
        s.inter_cnt[r] = 0u;
        s.code[p] = (uint8_t)kCmDropped;
        return;
    }
    if (r >= runs) return;
    const uint64_t j0 = s.prun_ev[r], j1 = s.prun_ev[r + 1u];
    const uint64_t key = keys[j0];
    const uint64_t cell = key >> kCmPixBits;
    const uint64_t a = cell / sh.ncubes;
    const uint32_t start_t = start0 + (uint32_t)a * sh.span;
    bool have_init = false;
    CmEv init{0u, 0u};
    if (r > 0u) {  // the previous non-empty pixel of the cube is the previous run, if that is of this cube
        const uint64_t jp = s.prun_ev[r - 1u];
        if ((keys[jp] >> kCmPixBits) == cell) {
            have_init = true;
            init = CmEv{s.sd[jp], s.st[jp]};
        }
    }
    const CmEv first{s.sd[j0], s.st[j0]};
    const uint8_t *__restrict__ sd = s.sd + j0;
    const uint32_t *__restrict__ st = s.st + j0;
    auto get = [&](uint64_t i) { return CmEv{sd[i], st[i]}; };
    if (!WRITE) {
        CmCountSink ci, cn;
        const uint32_t bs = cm_intra_pixel(ci, have_init, init, first, start_t);
        s.code[j0] = (uint8_t)bs;
        s.rt[j0] = first.t;
        uint8_t *code = s.code + j0;
        uint32_t *rt = s.rt + j0;
        cm_inter_pixel(cn, get, j1 - j0, start_t, sh.prm, [&](uint64_t i, uint32_t c, uint32_t t) {
            code[i] = (uint8_t)c;
            rt[i] = t;
        });
        s.intra_extra[r] = (uint32_t)(ci.n - 1u);
        s.inter_cnt[r] = (uint32_t)cn.n;
    } else {
        const CmAduBase b = cm_adu_base(sh, s, a);
        const uint64_t c = cell - a * sh.ncubes;
        // the cube run this pixel run lies in: cscan is exclusive, so it counts the run itself only behind its head
        const uint64_t q = (uint64_t)s.cscan[j0] + s.chead[j0] - 1u;
        const uint64_t intra_pos =
            b.sym + c + (q - b.crun0) * (uint64_t)(sh.npix - 1u) + (key & ((1u << kCmPixBits) - 1u)) + (s.sx[r] - b.sx0);
        const uint64_t inter_pos = b.sym + b.intra + (s.si[r] - b.si0);
        CmWriteSink wi{sym + intra_pos}, wn{sym + inter_pos};
        cm_intra_pixel(wi, have_init, init, first, start_t);
        cm_inter_pixel(wn, get, j1 - j0, start_t, sh.prm, CmNoNote());
    }
}

// per ADU a <= k: its first runs, its first kept event, its symbols (0 for the sentinel a == k)
__global__ __launch_bounds__(256) void cm_adu_kernel(CmShape sh, const uint64_t *__restrict__ keys, uint64_t p,
                                                     uint32_t k, CmScratch s) {
    const uint64_t a = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (a > k) return;
    const uint64_t e0 = cm_lower_bound(keys, 0, p, (a * sh.ncubes) << kCmPixBits);
    s.adu_prun[a] = s.pscan[e0];
    s.adu_crun[a] = s.cscan[e0];
    s.adu_recon_off[a] = s.kscan[e0];
    uint64_t cnt = 0;
    if (a < k) {
        const uint64_t e1 = cm_lower_bound(keys, e0, p, ((a + 1u) * sh.ncubes) << kCmPixBits);
        const uint32_t r0 = s.pscan[e0], r1 = s.pscan[e1];
        cnt = cm_adu_symbols(sh.ncubes, sh.npix, s.cscan[e1] - s.cscan[e0], s.sx[r1] - s.sx[r0], s.si[r1] - s.si[r0]);
    }
    s.adu_sym_cnt[a] = cnt;
}

// a block per (non-skipped cube, channel): the pixels of it that have no event
__global__ __launch_bounds__(256) void cm_empty_pixels_kernel(CmShape sh, const uint64_t *__restrict__ keys,
                                                              uint64_t runs_cube, CmScratch s,
                                                              uint16_t *__restrict__ sym) {
    const uint64_t q = blockIdx.x / sh.channels;
    if (q >= runs_cube) return;
    const uint32_t pix = (blockIdx.x % sh.channels) * 256u + threadIdx.x;
    const uint64_t j0 = s.crun_ev[q], j1 = s.crun_ev[q + 1u];
    const uint64_t cell = keys[j0] >> kCmPixBits;
    const uint64_t want = (cell << kCmPixBits) | pix;
    const uint64_t j = cm_lower_bound(keys, j0, j1, want);
    if (j < j1 && keys[j] == want) return;
    const uint64_t a = cell / sh.ncubes;
    const CmAduBase b = cm_adu_base(sh, s, a);
    const uint64_t c = cell - a * sh.ncubes;
    // j is the start of the next non-empty pixel's run (or of the next cube's first): the runs before it have grown
    sym[b.sym + c + (q - b.crun0) * (uint64_t)(sh.npix - 1u) + pix + (s.sx[s.pscan[j]] - b.sx0)] = cm_symbol_no_event();
}

// a lane per (ADU, cube): the cubes without an event; the ADU's start_t bytes and its eof
__global__ __launch_bounds__(256) void cm_cells_kernel(CmShape sh, const uint64_t *__restrict__ keys, uint64_t p,
                                                       uint64_t cells, uint32_t start0, CmScratch s,
                                                       uint16_t *__restrict__ sym) {
    const uint64_t cell = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (cell >= cells) return;
    const uint64_t a = cell / sh.ncubes, c = cell - a * sh.ncubes;
    const CmAduBase b = cm_adu_base(sh, s, a);
    const uint64_t j = cm_lower_bound(keys, 0, p, cell << kCmPixBits);
    if (!(j < p && (keys[j] >> kCmPixBits) == cell))  // j: the start of a later cube's run, or p
        sym[b.sym + c + (s.cscan[j] - b.crun0) * (uint64_t)(sh.npix - 1u) + (s.sx[s.pscan[j]] - b.sx0)] =
            cm_symbol_skip_cube();
    if (c == 0u) {
        CmWriteSink w{sym + s.adu_sym_off[a]};
        cm_put_start_t(w, start0 + (uint32_t)a * sh.span);
        sym[s.adu_sym_off[a + 1u] - 1u] = cm_symbol_eof();
    }
}

// the kept events with the t the decoder gets back, in its digest order (= the sorted order)
__global__ __launch_bounds__(256) void cm_recon_kernel(CmShape sh, const uint64_t *__restrict__ keys, uint64_t p,
                                                       CmScratch s, AdderEvent *__restrict__ recon) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j >= p || s.code[j] == kCmDropped) return;
    const uint64_t key = keys[j];
    const uint32_t pix = (uint32_t)(key & ((1u << kCmPixBits) - 1u));
    const uint64_t cube = (key >> kCmPixBits) % sh.ncubes;
    AdderEvent o;
    o.x = (uint16_t)((cube % sh.bx) * kCmBlock + pix % kCmBlock);
    o.y = (uint16_t)((cube / sh.bx) * kCmBlock + (pix / kCmBlock) % kCmBlock);
    o.c = sh.channels == 1u ? (uint8_t)ADDER_C_NONE : (uint8_t)(pix / 256u);
    o.d = s.sd[j];
    o.pad = 0;
    o.t = s.rt[j];
    recon[s.kscan[j]] = o;
}

// events per code: lane b of a wave counts code b by ballots; the block's four waves meet in LDS
__global__ __launch_bounds__(256) void cm_hist_kernel(const uint8_t *__restrict__ code, uint64_t p,
                                                      uint64_t *__restrict__ part) {
    __shared__ uint64_t w[4][kCmHistBins];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint64_t cnt = 0;
    const uint64_t stride = (uint64_t)gridDim.x * 256u;
    for (uint64_t base = (uint64_t)blockIdx.x * 256u + wave * 64u; base < p; base += stride) {  // wave-uniform
        const uint64_t j = base + lane;
        const uint32_t c = j < p ? code[j] : 0xFFu;
        for (uint32_t b = 0; b < kCmHistBins; ++b) {
            const uint64_t m = __ballot(c == b);
            if (lane == b) cnt += cm_popcount64(m);
        }
    }
    if (lane < kCmHistBins) w[wave][lane] = cnt;
    __syncthreads();
    if (threadIdx.x < kCmHistBins)
        part[(uint64_t)blockIdx.x * kCmHistBins + threadIdx.x] =
            w[0][threadIdx.x] + w[1][threadIdx.x] + w[2][threadIdx.x] + w[3][threadIdx.x];
}
__global__ __launch_bounds__(64) void cm_hist_sum_kernel(const uint64_t *__restrict__ part, uint32_t blocks,
                                                         CmCutResult *res) {
    if (threadIdx.x >= kCmHistBins) return;
    uint64_t sum = 0;
    for (uint32_t b = 0; b < blocks; ++b) sum += part[(uint64_t)b * kCmHistBins + threadIdx.x];
    res->hist[threadIdx.x] = sum;
}

struct CmWiden {
    __host__ __device__ __forceinline__ uint64_t operator()(uint32_t v) const { return v; }
};
struct CmKept {
    __host__ __device__ __forceinline__ uint32_t operator()(uint8_t c) const { return c != kCmDropped ? 1u : 0u; }
};
using CmWideIt = hipcub::TransformInputIterator<uint64_t, CmWiden, const uint32_t *>;
using CmKeptIt = hipcub::TransformInputIterator<uint32_t, CmKept, const uint8_t *>;

inline uint32_t cm_grid(uint64_t n) { return (uint32_t)((n + 255u) / 256u); }

}  // namespace

size_t cm_temp_bytes(uint64_t n) {
    size_t a = 0, b = 0, c = 0, d = 0, e = 0;
    const int m = (int)(n + 1u);
    hipcub::DoubleBuffer<uint64_t> k(nullptr, nullptr);
    hipcub::DoubleBuffer<uint32_t> v(nullptr, nullptr);
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, a, k, v, m);
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, b, (const uint32_t *)nullptr, (uint32_t *)nullptr, m);
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, c, CmWideIt(nullptr, CmWiden()), (uint64_t *)nullptr, m);
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, d, CmKeptIt(nullptr, CmKept()), (uint32_t *)nullptr, m);
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, e, (const uint64_t *)nullptr, (uint64_t *)nullptr, m);
    size_t t = a > b ? a : b;
    t = t > c ? t : c;
    t = t > d ? t : d;
    t = t > e ? t : e;
    return t + 256;
}

hipError_t cm_cut(const CmShape &sh, const AdderEvent *d_new, uint64_t n, uint32_t start_t, const CmScratch &s,
                  hipStream_t stream) {
    const uint64_t nchunks = (n + kCmChunk - 1u) / kCmChunk;
    if (n)
        hipLaunchKernelGGL(cm_chunk_kernel, dim3(cm_grid(n)), dim3(256), 0, stream, d_new, n, sh.width, sh.height,
                           sh.channels, s.bmax, s.bbad);
    hipLaunchKernelGGL(cm_walk_kernel, dim3(1), dim3(64), 0, stream, d_new, n, nchunks, s.bmax, s.bbad, start_t, sh.span,
                       s.cstart, s.cadu, s.res);
    if (n)
        hipLaunchKernelGGL(cm_number_kernel, dim3(cm_grid(n)), dim3(256), 0, stream, d_new, n, sh.span, s.bmax, s.cstart,
                           s.cadu, s.adu, s.res);
    return hipGetLastError();
}

hipError_t cm_group(const CmShape &sh, const AdderEvent *d_work, uint64_t carry, uint64_t p, uint32_t k,
                    const CmScratch &s, const uint64_t **keys, hipStream_t stream) {
    hipcub::DoubleBuffer<uint64_t> kb(s.keys0, s.keys1);
    hipcub::DoubleBuffer<uint32_t> vb(s.vals0, s.vals1);
    size_t tb = s.temp_bytes;
    hipError_t e = hipSuccess;
    if (p) {
        hipLaunchKernelGGL(cm_keys_kernel, dim3(cm_grid(p)), dim3(256), 0, stream, d_work, carry, p, s.adu, sh, s.keys0,
                           s.vals0);
        uint32_t bits = key_bits_for(((uint64_t)k * sh.ncubes) << kCmPixBits);
        if (bits > 64u) bits = 64u;
        e = hipcub::DeviceRadixSort::SortPairs(s.temp, tb, kb, vb, (int)p, 0, (int)bits, stream);
        if (e != hipSuccess) return e;
    }
    *keys = kb.Current();
    hipLaunchKernelGGL(cm_heads_kernel, dim3(cm_grid(p + 1u)), dim3(256), 0, stream, d_work, kb.Current(), vb.Current(),
                       p, s.sd, s.st, s.phead, s.chead);
    tb = s.temp_bytes;
    e = hipcub::DeviceScan::ExclusiveSum(s.temp, tb, (const uint32_t *)s.phead, s.pscan, (int)(p + 1u), stream);
    if (e != hipSuccess) return e;
    tb = s.temp_bytes;
    e = hipcub::DeviceScan::ExclusiveSum(s.temp, tb, (const uint32_t *)s.chead, s.cscan, (int)(p + 1u), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(cm_runs_kernel, dim3(cm_grid(p + 1u)), dim3(256), 0, stream, p, s);
    return hipGetLastError();
}

hipError_t cm_count(const CmShape &sh, const uint64_t *keys, uint64_t p, uint64_t runs_pixel, uint32_t k,
                    uint32_t start_t, const CmScratch &s, hipStream_t stream) {
    hipLaunchKernelGGL((cm_model_kernel<false>), dim3(cm_grid(runs_pixel + 1u)), dim3(256), 0, stream, sh, keys, p,
                       runs_pixel, start_t, s, (uint16_t *)nullptr);
    size_t tb = s.temp_bytes;
    hipError_t e = hipcub::DeviceScan::ExclusiveSum(s.temp, tb, CmWideIt(s.intra_extra, CmWiden()), s.sx,
                                                    (int)(runs_pixel + 1u), stream);
    if (e != hipSuccess) return e;
    tb = s.temp_bytes;
    e = hipcub::DeviceScan::ExclusiveSum(s.temp, tb, CmWideIt(s.inter_cnt, CmWiden()), s.si, (int)(runs_pixel + 1u),
                                         stream);
    if (e != hipSuccess) return e;
    tb = s.temp_bytes;
    e = hipcub::DeviceScan::ExclusiveSum(s.temp, tb, CmKeptIt(s.code, CmKept()), s.kscan, (int)(p + 1u), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(cm_adu_kernel, dim3(cm_grid((uint64_t)k + 1u)), dim3(256), 0, stream, sh, keys, p, k, s);
    tb = s.temp_bytes;
    e = hipcub::DeviceScan::ExclusiveSum(s.temp, tb, (const uint64_t *)s.adu_sym_cnt, s.adu_sym_off, (int)(k + 1u),
                                         stream);
    if (e != hipSuccess) return e;
    return hipGetLastError();
}

hipError_t cm_write(const CmShape &sh, const uint64_t *keys, uint64_t p, uint64_t runs_pixel, uint64_t runs_cube,
                    uint32_t k, uint32_t start_t, const CmScratch &s, uint16_t *d_sym, AdderEvent *d_recon,
                    hipStream_t stream) {
    if (runs_pixel)
        hipLaunchKernelGGL((cm_model_kernel<true>), dim3(cm_grid(runs_pixel)), dim3(256), 0, stream, sh, keys, p,
                           runs_pixel, start_t, s, d_sym);
    if (runs_cube)
        hipLaunchKernelGGL(cm_empty_pixels_kernel, dim3((uint32_t)(runs_cube * sh.channels)), dim3(256), 0, stream, sh,
                           keys, runs_cube, s, d_sym);
    const uint64_t cells = (uint64_t)k * sh.ncubes;
    if (cells)
        hipLaunchKernelGGL(cm_cells_kernel, dim3(cm_grid(cells)), dim3(256), 0, stream, sh, keys, p, cells, start_t, s,
                           d_sym);
    if (p) hipLaunchKernelGGL(cm_recon_kernel, dim3(cm_grid(p)), dim3(256), 0, stream, sh, keys, p, s, d_recon);
    uint32_t blocks = cm_grid(p);
    if (blocks > kCmHistBlocks) blocks = kCmHistBlocks;
    if (blocks) hipLaunchKernelGGL(cm_hist_kernel, dim3(blocks), dim3(256), 0, stream, s.code, p, s.hist_part);
    hipLaunchKernelGGL(cm_hist_sum_kernel, dim3(1), dim3(64), 0, stream, s.hist_part, blocks, s.res);
    return hipGetLastError();
}

}  // namespace adder
