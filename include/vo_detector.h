/*
 * vo_detector.h -- which detector the frame loop appends new features with: cv::FAST, as always, or the Shi-Tomasi detector of
 * vo_corners.h / vo_corners_response.h (cv::goodFeaturesToTrack).  The eighth header beside vo_hip.h.
 *
 * The reference's appendNewFeatures (feature.cpp:255-262) makes one detector call, featureDetectionFast; it ships
 * featureDetectionGoodFeaturesToTrack (feature.cpp:49-62) for the user who swaps that call.  vodet_set_params is that swap for the
 * three forms of the frame loop:
 *   synchronous   vo_detect_bucket (+ vo_track_frame);
 *   batch         VO_STAGE_DETECT of vo_batch_run;
 *   lock-step     vo_seq_*, with its look-ahead detection on the prepare stream and the inline detection of a step without it.
 * vo_fast_detect stays cv::FAST, and the vocorn_* / vocmask_* / voresp_* calls stay what they are.
 *
 * The detector is CONTEXT STATE, like vo_batch_set_detect_params.  vo_detect_params and every existing signature stay as they are:
 * fast_threshold / fast_nonmax are ignored under VODET_SHI_TOMASI; redetect_below, bucket_size and features_per_bucket apply as before.
 *
 * SEMANTICS UNDER VODET_SHI_TOMASI: the reference with the one call swapped.  When the carried set has fewer than redetect_below
 * points the list becomes "carried features, then the corners of goodFeaturesToTrack(image, max_corners, quality_level,
 * min_distance, noArray(), block_size, use_harris, k) in that call's own order" -- descending quality, equal qualities by descending
 * address -- with ages appended as zeros at the end of the ages vector (a longer ages vector behaves as under FAST, quirk B3);
 * bucketingFeatures follows with quirks B1-B3.  The image is the one FAST would read in the same call, in every context mode (kept
 * pair, input format, rectification).  With VODET_FAST every call returns the bytes it returned before this header existed.
 *
 * ERRORS.  The parameter checks are vocorn_*'s and voresp_*'s (VO_ERR_ARG, the same texts); an unknown detector is VO_ERR_ARG; a
 * refused record changes nothing.  vodet_set_params between vo_seq_configure and the end of the loop is VO_ERR_STATE: look-ahead
 * corners of the other detector may be in flight, and the schedule was probed with it.  A candidate list beyond the context's
 * corner-list capacity (vo_corners.h, CAPACITY) is never silent and travels the channel a FAST list overflow travels:
 * VO_ERR_OVERFLOW from vo_detect_bucket -- with nothing written --, VO_ERR_OVERFLOW from vo_batch_get_points, and the frame's
 * overflow flag (thus vo_seq_get_trajectory's VO_ERR_OVERFLOW) in the lock-step loop.
 *
 * SHARED BUFFERS.  The frame path runs in the candidate buffers the vocorn_* calls use (allocated on first use; the lock-step loop
 * takes its slots in vo_seq_configure, never inside a step).  After a frame-path detection vocorn_batch_get answers VO_ERR_STATE
 * until the next vocorn_batch_run; vocorn_detect and the other synchronous calls work as ever.
 *
 * SCHEDULES.  A Shi-Tomasi context neither reuses nor overwrites the schedules probed under FAST (the detector is part of the
 * probe's key), and the lock-step probe times the detector the loop will run.
 *
 * THE TOP-UP AWAY FROM THE CARRIED POINTS -- the same call under the disc mask of the points a frame carries in -- is vo_topup.h, the
 * ninth header; without it the call takes noArray().
 *
 * OUT OF SCOPE: a latency form of the map pass for one or a few images, and what vo_corners_response.h leaves out.
 */
#ifndef VO_DETECTOR_H
#define VO_DETECTOR_H

#include "vo_corners_response.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VODET_FAST 0
#define VODET_SHI_TOMASI 1

typedef struct vodet_params {
    int detector;           /* VODET_* */
    vocorn_params corners;  /* max_corners, quality_level, min_distance */
    voresp_params response; /* block_size, use_harris, k */
} vodet_params;

/* VODET_FAST; corners = vocorn_default_params, response = voresp_default_params */
void vodet_default_params(vodet_params *p);

/* The detector of the frame loop from now on.  p == NULL: the defaults.  Both records are checked whichever detector is named. */
int vodet_set_params(vo_ctx *ctx, const vodet_params *p);

/* The record in force. */
int vodet_get_params(const vo_ctx *ctx, vodet_params *p);

#ifdef __cplusplus
}
#endif
#endif /* VO_DETECTOR_H */
