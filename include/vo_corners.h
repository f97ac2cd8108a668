/*
 * vo_corners.h -- the Shi-Tomasi corner detector on the device: the reference's featureDetectionGoodFeaturesToTrack
 * (feature.cpp:49-62), the one helper of its feature.h that had no device path, and the detector that belongs with the two-image
 * tracker of vo_flow.h (whose GET_MIN_EIGENVALS err is the same score at the tracker's window).  The fifth header beside vo_hip.h.
 *
 *   vocorn_detect          cv::goodFeaturesToTrack(img, pts, max_corners, quality_level, min_distance, noArray(), 3, false, 0.04)
 *                          (blockSize 3, gradientSize 3, min eigenvalue): the same corners in the same order -- descending quality,
 *                          equal qualities by descending address -- as Point2f(x, y);
 *   vocorn_min_eigen_map   cv::cornerMinEigenVal(img, eig, 3, 3): the f32 quality map of the whole image, border pixels included;
 *   vocorn_batch_*         the detector over a range of the batch image table in one run (throughput mode).
 * Results are those of OpenCV 4.5 bit for bit as tests/host_check/corners_ref.c restates it (argued from upstream, not measured
 * against a linked OpenCV: tools/opencv_crosscheck.py does that where there is one).
 *
 * The context, vo_params.input_format (an image is converted to gray on its way in), byte strides, image sizes (32 x 32 up to the
 * context's maximum) and error codes are those of vo_hip.h; vo_last_error carries text; a NULL context is VO_ERR_ARG.  Images of a
 * synchronous call are never rectified (as vo_fast_detect: cv::goodFeaturesToTrack's counterpart takes the image it is given).
 * Inside the sequence loop (vo_seq_*) every call is VO_ERR_STATE.  Nothing is ever silently truncated.
 *
 * PARAMETERS.  max_corners == 0 means no limit.  OpenCV's CV_Assert conditions are VO_ERR_ARG: quality_level <= 0 (or NaN),
 * min_distance < 0 (or NaN), max_corners < 0.  A NULL params pointer means vocorn_default_params.
 * MIN_DISTANCE RANGE: 0 .. VOCORN_MAX_MIN_DISTANCE (256); beyond it VO_ERR_ARG.  Below 1 there is no suppression (OpenCV's
 * minDistance < 1 branch).  The bound is where the restatement stays exact and sensible: OpenCV tests dx * dx + dy * dy of integer
 * pixel offsets in f32, which is exact -- and so equal to the device's integer test -- while both offsets stay below 2 x the
 * cell of cvRound(min_distance) pixels, i.e. far below 2^24; and a 3 x 3 neighbourhood of 256-pixel cells already covers a
 * 768 x 768 area per candidate, past which the cell lists stop saving work.
 *
 * CAPACITY.  The candidate list (the thresholded local maxima, OpenCV's tmpCorners) is held in a list of the context's
 * corner-list capacity, the one vo_fast_detect documents: max(4 x max_pts, 16384, max_w x max_h / 16) per image.  More candidates
 * than that: VO_ERR_OVERFLOW, and nothing is written (vocorn_batch_get: for that image).
 *
 * THE IMAGE TABLE.  vocorn_detect and vocorn_min_eigen_map use the context's image table as vo_fast_detect does: the table is
 * configured for four images of this size (a table the batch API had configured is gone and is to be configured again; the kept
 * pair survives a call with an image of its own size), and the results of an earlier vocorn_batch_run can no longer be fetched
 * (vocorn_batch_get: VO_ERR_STATE).
 *
 * OUT OF SCOPE: gradientSize other than 3, block sizes other than 3 and 5.  The mask argument is in the sixth header,
 * vo_corners_mask.h; blockSize 5 and the Harris response (useHarrisDetector, k) in the seventh, vo_corners_response.h; the frame
 * loop (vo_detect_bucket, VO_STAGE_DETECT, vo_seq_*) detects with FAST like the reference's (visualOdometry.cpp:95-101) unless the
 * eighth, vo_detector.h, selects this detector for it -- the frame path then runs in the buffers of the calls here, and a
 * vocorn_batch_get after it answers VO_ERR_STATE until the next vocorn_batch_run.
 */
#ifndef VO_CORNERS_H
#define VO_CORNERS_H

#include "vo_hip.h"

#define VOCORN_MAX_MIN_DISTANCE 256

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vocorn_params {
    int max_corners;      /* 0: no limit */
    double quality_level; /* candidates are the local maxima above quality_level x the map's maximum */
    double min_distance;  /* pixels */
} vocorn_params;

/* 5000, 0.01, 5.0: the reference's call (feature.cpp:53-55) */
void vocorn_default_params(vocorn_params *p);

/* img: w x h of vo_params.input_format at byte stride `stride`; NULL: the left image of the pair the last vo_track_frame /
 * vo_circular_match kept (VO_ERR_STATE when the context holds none of this size).  *n_out: the corners found; it may exceed cap,
 * and then only the first cap are written to pts_out [cap][2] (vo_fast_detect's rule). */
int vocorn_detect(vo_ctx *ctx, const uint8_t *img, int w, int h, int stride, const vocorn_params *params, float *pts_out, int cap, int *n_out);

/* eig_out: h rows of w floats, eig_stride_floats (>= w) floats apart.  img as above. */
int vocorn_min_eigen_map(vo_ctx *ctx, const uint8_t *img, int w, int h, int stride, float *eig_out, int eig_stride_floats);

/* The detector on images first_image .. first_image + n_images - 1 of the batch image table (vo_batch_configure,
 * vo_batch_upload_image*: level 0 is all it reads, so no VO_STAGE_PYRAMID run is needed).  Enqueued on the context's stream like
 * any batch run; VO_ERR_STATE without a configured table, VO_ERR_ARG for a range outside it. */
int vocorn_batch_run(vo_ctx *ctx, const vocorn_params *params, int first_image, int n_images);

/* The corners of image image_idx of the latest vocorn_batch_run (waits for it): as vocorn_detect's outputs.  VO_ERR_STATE without
 * such a run on the table as configured now, VO_ERR_ARG for an image outside its range, VO_ERR_OVERFLOW as above. */
int vocorn_batch_get(vo_ctx *ctx, int image_idx, float *pts_out, int cap, int *n_out);

#ifdef __cplusplus
}
#endif
#endif /* VO_CORNERS_H */
