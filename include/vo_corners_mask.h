/*
 * vo_corners_mask.h -- the Shi-Tomasi detector of vo_corners.h with cv::goodFeaturesToTrack's `mask` argument, and the top-up a KLT
 * front end does with it: track the carried points (voflag_track), then detect new corners away from the survivors under a mask
 * with a disc punched out around each of them.  The sixth header beside vo_hip.h.
 *
 *   vocmask_detect         cv::goodFeaturesToTrack(img, pts, max_corners, quality_level, min_distance, mask, 3, false, 0.04);
 *   vocmask_disc_mask      the disc mask of a point list, built on the device, returned to the host;
 *   vocmask_replenish      that mask built on the device and the detector under it, in one call;
 *   vocmask_batch_*        masks for the images of the batch image table, and vocorn_batch_run under them (throughput mode: no
 *                          mask crosses the host link when it is built from kept points).
 *
 * WHAT A MASK DOES (OpenCV 4.5, featdetect.cpp; bit for bit as tests/corners_mask_cases.py restates it).  A mask is w x h bytes,
 * any non-zero byte means "allowed".  Nothing but the following changes relative to the maskless call:
 *   - the maximum that sets the threshold is minMaxLoc's over the allowed pixels only, border rows and columns included; with no
 *     allowed pixel it is 0;
 *   - threshold(TOZERO) and the 3 x 3 dilate run on the UNMASKED quality map: a stronger masked-out neighbour still suppresses an
 *     allowed pixel;
 *   - a local maximum is a candidate only where the mask is non-zero: only those enter the sort, the minDistance suppression and
 *     the count against the list capacity (VO_ERR_OVERFLOW).
 * An all-zero mask gives 0 corners and VO_OK.  Detecting without a mask and filtering afterwards gives other corners, for each of
 * the three reasons.
 *
 * The context, vo_params.input_format (an image is converted to gray on its way in), byte strides, image sizes (32 x 32 up to the
 * context's maximum) and error codes are those of vo_hip.h; vo_last_error carries text; a NULL context is VO_ERR_ARG.  Images of a
 * synchronous call are never rectified.  Inside the sequence loop (vo_seq_*) every call is VO_ERR_STATE.  Nothing is ever silently
 * truncated.  PARAMETERS, the MIN_DISTANCE RANGE, the CAPACITY rule, THE IMAGE TABLE and the kept image (img == NULL) are those of
 * vo_corners.h, word for word.
 *
 * MASKS are never format-converted or rectified: w x h bytes at mask_stride >= w, whatever the image's format; a smaller stride is
 * VO_ERR_ARG.
 *
 * THE DISC MASK, defined here (it is NOT cv::circle, whose filled outline differs by a few pixels per disc: a caller who wants
 * cv::circle's exact pixels passes a mask of their own).  All bytes start at 255.  Each kept point (x, y) contributes the centre
 * (cvRound(x), cvRound(y)), rounded half to even as lrintf does (2.5 -> 2, 3.5 -> 4, -0.5 -> 0); a point with a NaN or infinite
 * coordinate, or with |coordinate| >= 2^30, is skipped.  A pixel (px, py) of the image becomes 0 iff
 * (px - cx)^2 + (py - cy)^2 <= radius^2, in integers.  radius: 0 .. VOCORN_MAX_MIN_DISTANCE, beyond it VO_ERR_ARG; radius 0 clears
 * one pixel per point.  A centre outside the image still clears the part of its disc that lies inside.  n_kept == 0 gives an
 * all-255 mask.  kept_xy is [n_kept][2] floats; n_kept runs from 0 to the context's max_pts (beyond: VO_ERR_ARG), and kept_xy may
 * be NULL only when n_kept == 0.
 *
 * The device memory for the masks (one mask of max_w x max_h bytes and one point list per image of the table) is allocated by the
 * first vocmask_* call; a context that never makes one allocates and launches what it always did.
 *
 * OUT OF SCOPE: cv::circle-exact discs.  IN THE FRAME LOOP: vo_detector.h, the eighth header, puts this detector into
 * vo_detect_bucket, VO_STAGE_DETECT and vo_seq_*, and vo_topup.h, the ninth, runs it there under the disc mask of the points each
 * frame carries in.  blockSize 5 and the Harris response are in the seventh header, vo_corners_response.h, whose calls run
 * under these masks.  cv::FAST's own mask argument -- detect on the unmasked image, then drop what the mask forbids: the opposite
 * reading -- takes masks in this header's format and this header's disc mask, as a call and in the frame loop: vo_fast_mask.h, the tenth.
 */
#ifndef VO_CORNERS_MASK_H
#define VO_CORNERS_MASK_H

#include "vo_corners.h"

#ifdef __cplusplus
extern "C" {
#endif

/* vocorn_detect under `mask` (w x h bytes, mask_stride bytes apart).  mask == NULL: vocorn_detect itself, byte for byte, through
 * the same kernels (mask_stride is not looked at). */
int vocmask_detect(vo_ctx *ctx, const uint8_t *img, int w, int h, int stride, const uint8_t *mask, int mask_stride, const vocorn_params *params,
                   float *pts_out, int cap, int *n_out);

/* The disc mask of kept_xy for a w x h image (32 x 32 up to the context's maximum) into mask_out: h rows of w bytes, mask_stride
 * (>= w) bytes apart; bytes between the rows are left alone.  For callers who want to inspect or combine masks.  Like the other
 * synchronous calls it takes the image table (vo_corners.h, THE IMAGE TABLE). */
int vocmask_disc_mask(vo_ctx *ctx, int w, int h, const float *kept_xy, int n_kept, int radius, uint8_t *mask_out, int mask_stride);

/* "Replenish": the disc mask of kept_xy, built on the device, and vocorn_detect under it.  params applies as given: a caller who
 * wants `target` points in all passes max_corners = target - n_kept -- and, since max_corners == 0 means NO LIMIT (vo_corners.h),
 * does not call at all when nothing is needed. */
int vocmask_replenish(vo_ctx *ctx, const uint8_t *img, int w, int h, int stride, const float *kept_xy, int n_kept, int radius,
                      const vocorn_params *params, float *pts_out, int cap, int *n_out);

/* The mask of image image_idx of the batch image table (vo_batch_configure), for the vocmask_batch_run calls that follow: copied
 * from the host before the call returns.  mask == NULL removes the image's mask.  vo_batch_configure -- and with it every
 * synchronous call that takes the image table -- drops every mask.  VO_ERR_STATE without a configured table, VO_ERR_ARG for an
 * image outside it. */
int vocmask_batch_set_mask(vo_ctx *ctx, int image_idx, const uint8_t *mask, int mask_stride);

/* ... built on the device as the disc mask of kept_xy (copied before the call returns; the mask itself is built on the context's
 * stream, in order with the runs). */
int vocmask_batch_set_kept(vo_ctx *ctx, int image_idx, const float *kept_xy, int n_kept, int radius);

/* vocorn_batch_run under the masks set so far: an image without a mask runs unmasked.  Results come through vocorn_batch_get. */
int vocmask_batch_run(vo_ctx *ctx, const vocorn_params *params, int first_image, int n_images);

#ifdef __cplusplus
}
#endif
#endif /* VO_CORNERS_MASK_H */
