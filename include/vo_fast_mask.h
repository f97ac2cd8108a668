/*
 * vo_fast_mask.h -- cv::FAST UNDER A MASK: FastFeatureDetector::detect's mask argument as a call of its own, and the frame loop's
 * top-up away from the carried points for the reference's own detector (VODET_FAST, vo_detector.h).  The tenth header beside vo_hip.h.
 *
 *   vofm_detect      FastFeatureDetector::create(threshold, nonmax)->detect(img, keypoints, mask) + KeyPoint::convert;
 *   vofm_replenish   the disc mask of a point list (vo_corners_mask.h), built on the device, and the detector under it, in one call;
 *   vofm_set_params  the same inside appendNewFeatures' cv::FAST call of the frame loop, under the disc mask of the carried points.
 *
 * WHAT A MASK DOES (OpenCV 4.5, features2d: fast.cpp, keypoint.cpp).  detect(image, keypoints, mask) is
 *     FAST(image, keypoints, threshold, nonmax);  KeyPointsFilter::runByPixelsMask(keypoints, mask);
 * a keypoint is dropped iff mask((int)(pt.y + 0.5f), (int)(pt.x + 0.5f)) == 0, and the survivors keep their (row-major) order.
 * Non-maximum suppression runs on the UNMASKED image: a corner its neighbour suppressed does not come back when that neighbour is
 * masked out.  Detect-then-filter IS the definition here -- the opposite of goodFeaturesToTrack's mask (vo_corners_mask.h), where
 * filtering afterwards is the wrong reading.  An all-zero mask gives 0 corners and VO_OK.
 *
 * MASKS follow vo_corners_mask.h: w x h bytes, any non-zero byte means "allowed", mask_stride >= w (smaller: VO_ERR_ARG), never
 * format-converted or rectified.  THE DISC MASK, its centre rounding, the skipped points (NaN, +-inf, |coordinate| >= 2^30), the radius
 * range 0 .. VOCORN_MAX_MIN_DISTANCE and n_kept == 0 (an all-255 mask) are that header's definition; kept_xy is [n_kept][2] floats,
 * n_kept runs from 0 to the context's max_pts (beyond: VO_ERR_ARG).
 *
 * The context, image sizes, byte strides, the kept left image (img == NULL) and the error codes are vo_fast_detect's (vo_hip.h); a NULL
 * context is VO_ERR_ARG; inside the sequence loop (vo_seq_*) the synchronous calls are VO_ERR_STATE.  Like vo_fast_detect, vofm_detect
 * and vofm_replenish take the image table (a one-frame configuration) and frame 0's feature list: features a batch-API user set with
 * vo_batch_set_features, and the plane vofm_get_mask would have returned, do not survive such a call.
 *
 * CAPACITY.  The filter reads cv::FAST's list from the context's corner list, so VO_ERR_OVERFLOW is judged on the UNMASKED list
 * against that list's capacity (max(4 x max_pts, 16384, max_w x max_h / 16)), whatever the mask leaves of it: vofm_detect then
 * writes nothing and sets *n_out to the unmasked count; in the frame loop the frame's overflow flag travels the channels
 * vo_detect_bucket (VO_ERR_OVERFLOW, nothing written), the batch stage and the lock-step loop already name.
 *
 * IN THE FRAME LOOP: the reference with one call changed.  With mode VOFM_CARRIED and the detector VODET_FAST, a frame whose carried
 * set has fewer than redetect_below points gets
 *     mask = THE DISC MASK (vo_corners_mask.h) of currentVOFeatures.points at entry, radius `radius`
 *     FastFeatureDetector::create(fast_threshold, fast_nonmax)->detect(image, keypoints, mask)
 *     corners appended in FAST's own order, ages as zeros behind a possibly longer ages vector (quirk B3)
 * and bucketingFeatures follows with quirks B1-B3.  An empty carried set is the unmasked call, byte for byte; a mask that allows
 * nothing gives 0 new points and no error; n_new and the info rows count the masked list.  In all three forms of the loop:
 * vo_detect_bucket, VO_STAGE_DETECT of vo_batch_run, and vo_seq_* -- there the look-ahead keeps computing the unmasked list of each
 * ring slot (which no mask changes) one step early, and the step draws the discs and filters that list once the carried sets are
 * known.  With VOFM_OFF every call launches what it launched and returns the bytes it returned before this header.
 *
 * The record is CONTEXT STATE with votop_set_params' rules (vo_topup.h): an unknown mode or a radius outside
 * 0 .. VOCORN_MAX_MIN_DISTANCE is VO_ERR_ARG and changes nothing; between vo_seq_configure and the end of the loop vofm_set_params is
 * VO_ERR_STATE; NULL params means the defaults.  Under VODET_SHI_TOMASI the record is stored and has no effect (that detector's
 * top-up is votop_*, which in turn has no effect under VODET_FAST).
 *
 * MEMORY.  Per frame one plane of max_w x max_h bytes (the context's maximum, rounded up to 16) and two corner lists of the context's
 * corner-list capacity, 8 bytes an entry -- the unmasked list of a detection made inside the step and the list under the mask: from
 * the context's owner when a run with the record on first needs them (vo_seq_configure, for all its sequences, the first list too,
 * since a step without look-ahead corners detects inline; the batch stage when a run covers more frames than any before it; the first
 * vofm_detect / vofm_replenish, for one frame), never inside a step.  At 1241 x 376 and max_pts 4096 that is 0.47 MB + 2 x 0.23 MB
 * per frame, 240 MB for 256 sequences.  A context that never turns the record on and never makes a vofm_* call allocates and
 * launches what it always did.  SCHEDULES: the mode is part of the probe's key, like the detector and votop's mode.
 *
 * OUT OF SCOPE: a per-frame corner budget (retainBest's order depends on std::nth_element: there is nothing to be bit-exact to),
 * cv::circle-exact discs (a caller who wants them passes a mask of their own to vofm_detect), and any change to votop_*.
 */
#ifndef VO_FAST_MASK_H
#define VO_FAST_MASK_H

#include "vo_topup.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VOFM_OFF 0
#define VOFM_CARRIED 1

typedef struct vofm_params {
    int mode;   /* VOFM_* */
    int radius; /* 0 .. VOCORN_MAX_MIN_DISTANCE */
} vofm_params;

/* vo_fast_detect under `mask` (w x h bytes, mask_stride bytes apart): corners in row-major order, *n_out the masked count (it may
 * exceed cap: only the first cap corners are written).  mask == NULL: vo_fast_detect itself, byte for byte (mask_stride must then
 * be 0). */
int vofm_detect(vo_ctx *ctx, const uint8_t *img, int w, int h, int stride, int threshold, int nonmax, const uint8_t *mask, int mask_stride,
                float *pts_out, int cap, int *n_out);

/* "Replenish": the disc mask of kept_xy, built on the device, and vofm_detect under it. */
int vofm_replenish(vo_ctx *ctx, const uint8_t *img, int w, int h, int stride, int threshold, int nonmax, const float *kept_xy, int n_kept,
                   int radius, float *pts_out, int cap, int *n_out);

/* VOFM_OFF, radius 5 */
void vofm_default_params(vofm_params *p);

/* cv::FAST's mask in the frame loop from now on.  p == NULL: the defaults. */
int vofm_set_params(vo_ctx *ctx, const vofm_params *p);

/* The record in force. */
int vofm_get_params(const vo_ctx *ctx, vofm_params *p);

/* The mask plane (h rows of w bytes, mask_stride apart) the last vo_detect_bucket (frame 0) or VO_STAGE_DETECT built for `frame`.
 * VO_ERR_STATE inside the sequence loop, when no masked detection has run on the table as it is configured, and for a frame that
 * did not detect again. */
int vofm_get_mask(vo_ctx *ctx, int frame, uint8_t *mask_out, int mask_stride);

#ifdef __cplusplus
}
#endif
#endif /* VO_FAST_MASK_H */
