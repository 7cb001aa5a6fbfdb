// adder_compressed_kernels.h -- the launches of adder_compressed_model.hip: the compressed codec's source model over
// events in HBM.  adder_compressed_model_api.cpp owns the buffers and the order of the steps; every output
// position comes from a scan, so no kernel here uses an atomic.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/adder_hip.h"
#include "adder_compressed_logic.hpp"

namespace adder {

struct CmShape {
    uint32_t width, height, channels;
    uint32_t bx, by;    // cubes per row, rows of cubes
    uint64_t ncubes;    // bx * by
    uint32_t npix;      // channels * 256
    uint32_t span;      // ref_interval * adu_interval (u32, as the host encoder has it)
    CmParams prm;
};

constexpr uint32_t kCmChunk = 64;      // events a wave resolves the ADU cut of
constexpr uint32_t kCmHistBlocks = 256;
constexpr uint32_t kCmHistBins = 17;   // bit shift 0..15, dropped

struct CmCutResult {  // what the cut leaves for the host
    uint32_t k;        // ADUs the call's events close
    uint32_t start_t;  // of the ADU left open
    uint32_t bad;      // an event outside the plane or channel
    uint32_t pad;
    uint64_t p_new;    // the first event of the open ADU (meaningful when k > 0)
    uint64_t runs_pixel, runs_cube;  // (filled by cm_runs)
    uint64_t hist[kCmHistBins];      // (filled by cm_hist)
};

struct CmScratch {  // for `cap` events (+1 sentinel each), `adu_cap` ADUs (+1), reserved by the api
    // the cut, over the call's new events
    uint32_t *bmax, *bbad, *cstart, *cadu;  // per chunk of kCmChunk events
    uint32_t *adu;                          // per new event: ADUs closed up to and including it
    // grouping, over the events of the ADUs a call closes (sorted order from here on)
    uint64_t *keys0, *keys1;
    uint32_t *vals0, *vals1;
    uint8_t *sd;      // d
    uint32_t *st;     // t
    uint32_t *rt;     // reconstructed t
    uint8_t *code;    // bit shift 0..15, kCmDropped
    uint32_t *phead, *chead, *pscan, *cscan, *kscan;  // run-start flags; their exclusive sums; that of the kept flags
    uint32_t *prun_ev, *crun_ev;                      // the sorted index a pixel / cube run starts at
    uint32_t *intra_extra, *inter_cnt;                // per pixel run: intra symbols beyond the pixel's one; inter symbols
    uint64_t *sx, *si;                                // their exclusive sums
    // per ADU
    uint32_t *adu_prun, *adu_crun;  // first pixel / cube run
    uint64_t *adu_recon_off, *adu_sym_cnt, *adu_sym_off;
    uint64_t *hist_part;            // kCmHistBlocks * kCmHistBins
    void *temp;
    size_t temp_bytes;
    CmCutResult *res;
};

// what hipcub's sort and scans take for n events
size_t cm_temp_bytes(uint64_t n);

// ADU index of n new events in stream order, from start_t; s.res gets k, start_t, bad, p_new
hipError_t cm_cut(const CmShape &sh, const AdderEvent *d_new, uint64_t n, uint32_t start_t, const CmScratch &s,
                  hipStream_t stream);
// keys of events [0, p) of d_work (the first `carry` are of ADU 0, the others take s.adu), the stable sort, the
// gather of d and t, run starts and their scans; s.res gets the run counts.  -> the sorted keys through *keys
hipError_t cm_group(const CmShape &sh, const AdderEvent *d_work, uint64_t carry, uint64_t p, uint32_t k,
                    const CmScratch &s, const uint64_t **keys, hipStream_t stream);
// the model, counting: per pixel run the symbols, per event its code and reconstructed t; then per ADU the symbol
// and event offsets (k + 1 entries: the last is the total)
hipError_t cm_count(const CmShape &sh, const uint64_t *keys, uint64_t p, uint64_t runs_pixel, uint32_t k,
                    uint32_t start_t, const CmScratch &s, hipStream_t stream);
// the model again, writing: d_sym (the counted total of words) and d_recon (the kept events); s.res gets the histogram
hipError_t cm_write(const CmShape &sh, const uint64_t *keys, uint64_t p, uint64_t runs_pixel, uint64_t runs_cube,
                    uint32_t k, uint32_t start_t, const CmScratch &s, uint16_t *d_sym, AdderEvent *d_recon,
                    hipStream_t stream);

}  // namespace adder
