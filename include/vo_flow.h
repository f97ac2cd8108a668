/*
 * vo_flow.h -- the two-image sparse optical-flow calls of libvo_hip.so, beside the C ABI of vo_hip.h.
 *
 * The reference exports a second tracker next to circularMatching(): featureTracking(img_1, img_2, points1, points2, status)
 * (feature.h:52, feature.cpp:64-74) = ONE cv::calcOpticalFlowPyrLK(img_1, img_2, points1, points2, status, err, Size(21, 21), 3,
 * TermCriteria(COUNT + EPS, 30, 0.01), 0, 0.001) followed by deleteUnmatchFeatures (feature.cpp:20-37).  These calls are that:
 * positions, status and the err residual of plain pyramidal Lucas-Kanade between two images, which vo_circular_match does not
 * return (four images, no err, a feature retires as soon as a later filter would drop it).  A mono front end is then host glue:
 * vo_fast_detect, voflow_feature_tracking, vo_essential_pose.
 *
 * Everything of vo_hip.h holds here: the same vo_ctx (one per host thread per GPU), the same VO_OK / VO_ERR_* codes with
 * vo_last_error(), points as interleaved float32 (x, y), caller-allocated outputs, no exceptions.  Images are read as
 * vo_params.input_format says (byte stride, sub-views as everywhere).  The LK parameters are the context's vo_params:
 * lk_max_level, lk_max_count, lk_epsilon, lk_min_eig_threshold; the window is 21 x 21 (vo_flow_win.h: the same calls with a
 * window of 5 x 5 .. 21 x 21).
 *
 * RESULTS, bit for bit those of OpenCV's CPU tracker with an err vector requested: next_pts, status (1 tracked, 0 not) and
 *   err = sum over the 21 x 21 window of |J(final position) - I| / (32 * 21 * 21)      (flags 0: the L1 residual per pixel)
 * of a point with status 1; a point that ends with status 0 for any reason has err 0.  status is the one of a call WITH err,
 * whether err is passed or not (the final in-bounds check of that block applies).  A start point with a NaN coordinate, +-inf or
 * a value beyond int32 fails with status 0 and its reported position is the propagated (NaN / huge) value, as documented for
 * vo_circular_match.
 *
 * RECTIFICATION (vo_params.rectify): the synchronous calls remap BOTH images through the LEFT maps -- mono tracking runs on the
 * left camera.  The batch calls read the image table, whose uploads keep their rule (even index = left, odd = right).
 *
 * KEPT PAIR: a synchronous call here uses the image slots of the drop-in calls of vo_hip.h.  Afterwards the context holds NO kept
 * pair: vo_kept_pair_id() returns 0 and a stereo call without t0 images answers VO_ERR_STATE.  As after any drop-in call, the
 * batch API's table is to be configured / its quads and pairs set again before the next vo_batch_run / voflow_batch_run.
 *
 * ERRORS: VO_ERR_ARG -- NULL context, image, points or required output; n < 0 or beyond max_pts; an image size beyond
 * vo_create's (or below 32); a stride below w * bytes per pixel; a pair index outside the image table; a frame beyond the
 * configured frames.  n == 0 returns VO_OK and writes nothing.  VO_ERR_STATE -- inside the lock-step loop (vo_seq_*);
 * voflow_batch_run without a configured table, without pairs, or on an image uploaded after its pyramid was last built.
 */
#ifndef VO_FLOW_H
#define VO_FLOW_H

#include "vo_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* cv::calcOpticalFlowPyrLK(prev, next, prev_pts, next_pts, status, err, Size(21, 21), lk_max_level,
 * TermCriteria(COUNT + EPS, lk_max_count, lk_epsilon), 0, lk_min_eig_threshold).
 * prev_pts_xy / next_pts_xy [n][2], status [n], err [n] or NULL (not computed). */
int voflow_track(vo_ctx *ctx, const uint8_t *prev, const uint8_t *next, int w, int h, int stride, const float *prev_pts_xy, int n,
                 float *next_pts_xy, uint8_t *status, float *err);

/* featureTracking() (feature.cpp:64-74): the call above + deleteUnmatchFeatures.  Point i survives iff status[i] != 0 and its
 * tracked position has no negative coordinate.  pts0_io [n][2]: the n start points in, the *n_out survivors out; pts1_out
 * [n][2]: their tracked positions (*n_out rows written); status [n]: as the reference leaves it -- NOT compacted, and 0 where a
 * tracked point was dropped for a negative coordinate; err [n] or NULL: not compacted; keep_idx [n] or NULL: index of every
 * survivor among the n start points (*n_out entries, increasing). */
int voflow_feature_tracking(vo_ctx *ctx, const uint8_t *prev, const uint8_t *next, int w, int h, int stride, float *pts0_io, int n,
                            float *pts1_out, uint8_t *status, float *err, int32_t *keep_idx, int *n_out);

/* Throughput mode, on the image table of the batch API as it is: vo_batch_configure, vo_batch_upload_image(_dev),
 * vo_batch_run(VO_STAGE_PYRAMID), vo_batch_set_points(frame, ...) and vo_batch_sync.  Frame f tracks its points from image
 * pairs2[2 f] to image pairs2[2 f + 1]; n_frames = the configured frame count.  voflow_batch_run is asynchronous on the
 * context's stream; voflow_batch_get waits for it and copies the first n results of a frame (any output may be NULL). */
int voflow_batch_set_pairs(vo_ctx *ctx, const int32_t *pairs2, int n_frames);
int voflow_batch_run(vo_ctx *ctx);
int voflow_batch_get(vo_ctx *ctx, int frame, float *next_pts_xy, uint8_t *status, float *err, int n);

#ifdef __cplusplus
}
#endif
#endif /* VO_FLOW_H */
