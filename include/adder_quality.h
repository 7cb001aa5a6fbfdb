/* adder_quality.h -- C-ABI of the reconstruction quality metrics (libadder_hip.so).
 *
 * calculate_quality_metrics of the reference (adder-codec-rs/src/utils/cv.rs:306-430) on the device, for n pairs of
 * u8 frames [H][W][C] (C = 1 or 3, interleaved -- the layout of the transcoder's input batches, of
 * adder_framer_pop_device and of the running-intensities plane):
 *   MSE  = sum of (a - b)^2 over every element / (H * W * C), an MSE of exactly 0 reported as 1e-7;
 *   PSNR = 20 log10(255) - 10 log10(MSE), evaluated on the host with the platform libm;
 *   SSIM = per channel, every 8x8 window at stride 1: r = ((2 mx my + C1)(2 cov + C2)) / ((mx^2 + my^2 + C1)(vx + vy + C2)),
 *          the channel score sum(64 r) / sum(64), the frame's (sum of scores / C) * 100.  NaN when H < 8 or W < 8.
 * MSE (and so PSNR) equals the reference bit for bit.  Each window's r equals the reference's bit for bit; the sum over
 * the windows is a fixed-order tree, within the first-order rounding bound of the reference's sequential sum
 * (DESIGN 5h).  A frame's results do not depend on the run or on the other frames of the call. */
#ifndef ADDER_QUALITY_H
#define ADDER_QUALITY_H

#include <stddef.h>
#include <stdint.h>

#include "adder_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ADDER_QUALITY_ABI_VERSION 1u

/* Metrics mask: QualityMetrics' Some / None (cv.rs:283-293) */
enum { ADDER_QUALITY_MSE = 1, ADDER_QUALITY_PSNR = 2, ADDER_QUALITY_SSIM = 4 };

typedef struct AdderQualityParams {
    uint32_t abi_version; /* = ADDER_QUALITY_ABI_VERSION */
    uint16_t width;
    uint16_t height;
    uint8_t channels;     /* 1 or 3 */
    uint8_t metrics;      /* ADDER_QUALITY_* mask, not empty */
    uint16_t reserved0;
    int32_t device_id;
} AdderQualityParams;

typedef struct AdderQualityResult {
    double mse;
    double psnr;
    double ssim;          /* in percent, as the reference reports it */
    uint32_t present;     /* ADDER_QUALITY_* mask of the fields filled; the others are 0 */
    uint32_t reserved;
} AdderQualityResult;

typedef struct AdderQuality AdderQuality;

/* ADDER_E_BAD_PARAMS: abi_version, a zero dimension, channels not 1 or 3, an empty mask.  ADDER_E_NO_DEVICE without
 * a gfx950 device (no CPU fallback). */
int adder_quality_create(const AdderQualityParams *p, AdderQuality **out);
void adder_quality_destroy(AdderQuality *q);
/* Describes the last failure of `q` (or of the last failed create when q is null). */
const char *adder_quality_last_error(const AdderQuality *q);
/* Elements of the per-window map of n frames: n * C * (H - 7) * (W - 7) doubles, channel-major ([n][C][H-7][W-7],
 * the reference's window order within a channel); 0 when the plane has no window. */
uint64_t adder_quality_map_elems(const AdderQuality *q, uint32_t n_frames);

/* n_frames pairs in device memory, frame k at byte k * H * W * C of each.  Queued on `stream` (NULL: the default
 * stream) behind whatever is queued there already; waits for its own results and fills out[0 .. n_frames).
 * d_ssim_map: NULL, or a device buffer of adder_quality_map_elems doubles that receives every window's r (SSIM must
 * be in the mask).  Every argument is checked before anything is launched. */
int adder_quality_compute_device(AdderQuality *q, const uint8_t *d_original, const uint8_t *d_reconstructed,
                                 uint32_t n_frames, AdderQualityResult *out, double *d_ssim_map, void *stream);
/* The same for frames in host memory: copies in, computes on the device, copies the map (if not NULL) out. */
int adder_quality_compute_host(AdderQuality *q, const uint8_t *original, const uint8_t *reconstructed,
                               uint32_t n_frames, AdderQualityResult *out, double *ssim_map);

#ifdef __cplusplus
}
#endif
#endif /* ADDER_QUALITY_H */
