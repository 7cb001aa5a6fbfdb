/* adder_fast.h -- C-ABI of the dense FAST 9_16 detector and of the feature precision / recall / accuracy
 * (libadder_hip.so).
 *
 * The reference's feature log (video.rs:926-1060, feature "feature-logging") runs the frame-based FAST detector over
 * the whole running-intensities plane after every frame and scores the event-driven features against it with
 * feature_precision_recall_accuracy (utils/cv.rs:235-279).  Here, for n u8 frames [H][W][C] (C = 1 or 3, interleaved;
 * channel 0 of a pixel is the one examined, the plane the event detectors read, cv.rs:61-67):
 *   corner: a pixel at least 3 from every border with 9 circularly contiguous pixels of the radius-3 circle
 *           (cv.rs:25-30 CIRCLE3) all > centre + threshold, or all < centre - threshold;
 *   score : max over both directions and the 16 arcs of (min over the arc of the signed difference) - 1, the largest
 *           threshold at which the pixel is still a corner: threshold .. 254 for a corner, 0 for any other pixel;
 *   nonmax: a corner is kept iff its score is strictly greater than the score of each of its 8 neighbours (a pixel
 *           outside the plane counts as 0); without nonmax every corner is kept.
 * At threshold 30 the corners are the pixels the event detectors (adder_hip_update_detect_features,
 * adder_framer_detect_features, the adder-viz player) call features.  The counts of a scoring cover all W * H
 * positions, and the ratios are the reference's f64 divisions: 0 / 0 is NaN and is not replaced.  Where the reference
 * looks predictions up by Coord{c: None}, so that nothing matches in a three-channel video, this library compares
 * positions. */
#ifndef ADDER_FAST_H
#define ADDER_FAST_H

#include <stddef.h>
#include <stdint.h>

#include "adder_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ADDER_FAST_ABI_VERSION 1u
#define ADDER_FAST_DEFAULT_THRESHOLD 30u /* cv.rs:22 INTENSITY_THRESHOLD */

typedef struct AdderFastParams {
    uint32_t abi_version; /* = ADDER_FAST_ABI_VERSION */
    uint16_t width;
    uint16_t height;
    uint8_t channels;     /* 1 or 3 */
    uint8_t threshold;    /* 1 .. 255; 0 is refused: the score could not tell a score-0 corner from a non-corner */
    uint8_t nonmax;       /* 0 or 1 */
    uint8_t reserved0;
    int32_t device_id;
} AdderFastParams;

typedef struct AdderFastEval {
    uint64_t tp, fp, tn, fn; /* over all W * H positions, borders included (cv.rs:258-273) */
    uint64_t gt_count;       /* kept pixels of the dense detector */
    uint64_t pred_count;     /* predicted positions */
    double precision;        /* tp / (tp + fp) */
    double recall;           /* tp / (tp + fn) */
    double accuracy;         /* (tp + tn) / (tp + tn + fp + fn) */
} AdderFastEval;

typedef struct AdderFast AdderFast;

/* ADDER_E_BAD_PARAMS: abi_version, a zero dimension, a plane of 2^31 positions or more, channels not 1 or 3,
 * threshold 0, nonmax above 1.  ADDER_E_NO_DEVICE without a gfx950 device (no CPU fallback). */
int adder_fast_create(const AdderFastParams *p, AdderFast **out);
void adder_fast_destroy(AdderFast *f);
/* Describes the last failure of `f` (or of the last failed create when f is null). */
const char *adder_fast_last_error(const AdderFast *f);

/* Detects over n_frames frames in device memory, frame k at byte k * H * W * C.  Queued on `stream` (NULL: the
 * default stream) behind whatever is queued there already; waits for its own results.
 *   d_mask  [n][H][W] u8, 1 = kept, or NULL;
 *   d_score [n][H][W] u8, or NULL;
 *   d_xy    the kept pixels as x | y << 16 (the packing of adder_hip_feature_detect), in raster order within a frame
 *           and frame after frame, room for `capacity` of them, or NULL;
 *   counts  [n] in host memory, always filled.
 * When d_xy is given and the total exceeds `capacity` the call returns ADDER_E_OUT_CAPACITY: nothing is written to
 * d_xy, the counts (and mask and score) are valid.  Every argument is checked before anything is launched.  No device
 * memory is allocated once the context has seen a call of the same n_frames and outputs. */
int adder_fast_detect_device(AdderFast *f, const uint8_t *d_frames, uint32_t n_frames, uint8_t *d_mask,
                             uint8_t *d_score, uint32_t *d_xy, uint64_t capacity, uint64_t *counts, void *stream);
/* The same for frames and outputs in host memory. */
int adder_fast_detect_host(AdderFast *f, const uint8_t *frames, uint32_t n_frames, uint8_t *mask, uint8_t *score,
                           uint32_t *xy, uint64_t capacity, uint64_t *counts);

/* Clears one [H][W] plane in device memory and sets 1 at each of the n packed coordinates (x | y << 16) of d_xy, so
 * that a feature list (adder_hip_feature_detect, the framer's, the viz player's) can be scored.  Duplicates are
 * harmless.  A coordinate outside the plane: ADDER_E_BAD_PARAMS, and the plane is not written at all. */
int adder_fast_mask_from_xy_device(AdderFast *f, const uint32_t *d_xy, uint64_t n, uint8_t *d_mask, void *stream);

/* Detects over n_frames frames and scores d_prediction ([n][H][W] u8, nonzero = predicted) against the kept pixels:
 * out[0 .. n_frames) in host memory. */
int adder_fast_evaluate_device(AdderFast *f, const uint8_t *d_frames, const uint8_t *d_prediction, uint32_t n_frames,
                               AdderFastEval *out, void *stream);
int adder_fast_evaluate_host(AdderFast *f, const uint8_t *frames, const uint8_t *prediction, uint32_t n_frames,
                             AdderFastEval *out);

#ifdef __cplusplus
}
#endif
#endif /* ADDER_FAST_H */
