/*
 * vo_topup.h -- the frame loop's top-up AWAY FROM THE CARRIED POINTS: under VODET_SHI_TOMASI (vo_detector.h) appendNewFeatures'
 * goodFeaturesToTrack call takes the disc mask of the points the frame carries in (vo_corners_mask.h).  The ninth header beside
 * vo_hip.h.
 *
 * SEMANTICS: the reference with one call changed.  With mode VOTOP_CARRIED and the detector VODET_SHI_TOMASI, a frame whose carried
 * set has fewer than redetect_below points gets
 *     mask = THE DISC MASK (vo_corners_mask.h) of currentVOFeatures.points, radius `radius`
 *     goodFeaturesToTrack(image, corners, max_corners, quality_level, min_distance, mask, block_size, use_harris, k)
 *     corners appended in that call's own order, ages as zeros behind a possibly longer ages vector (quirk B3)
 * and bucketingFeatures follows with quirks B1-B3, as without the top-up.
 *   disc centres     every carried point at entry, whatever its age: the first n_tracked of the list
 *   skipped points   vo_corners_mask.h's rule: NaN, +-inf and |coordinate| >= 2^30
 *   empty carried set  the unmasked call, byte for byte
 *   mask that allows nothing  0 corners, no error
 *   mask semantics   vocmask_detect's: the maximum over the allowed pixels (border included, 0 with none), threshold and dilate on the
 *                    unmasked map, only allowed maxima enter the sort, the minDistance loop and the capacity count
 *   max_corners      as given (no per-frame budget)
 *   image            the one FAST would read in the same call, in every context mode
 * In all three forms of the loop: vo_detect_bucket, VO_STAGE_DETECT of vo_batch_run, and vo_seq_* -- there the look-ahead computes the
 * response map (which no mask changes) one step early and the step finishes the call once the carried sets are known.
 * Under VODET_FAST, or with VOTOP_OFF, every call launches what it launched and returns the bytes it returned before this header.
 *
 * The record is CONTEXT STATE, like vodet_set_params.  An unknown mode or a radius outside 0 .. VOCORN_MAX_MIN_DISTANCE is
 * VO_ERR_ARG and changes nothing; between vo_seq_configure and the end of the loop votop_set_params is VO_ERR_STATE (the loop took its
 * planes and probed its schedule with the record in force); a NULL context is VO_ERR_ARG.  Under VODET_FAST the record is stored
 * and has no effect.  A candidate list beyond the capacity travels the channels vo_detector.h names.
 *
 * MEMORY.  One w x h byte plane per frame and, in the lock-step loop, one map per sequence and ring slot: from the context's owner
 * when a run with the top-up on first needs them (vo_seq_configure; the batch stage where it grows the candidate buffers), never
 * inside a step.  A context that never turns the top-up on allocates and launches what it always did.
 *
 * SCHEDULES.  The mode is part of the probe's key, like the detector: schedules probed without the top-up are neither reused nor
 * overwritten, and the lock-step probe times what the loop will run.
 *
 * OUT OF SCOPE: a per-frame corner budget (target - n_carried), cv::circle-exact discs, and a latency form of the map pass for one or a
 * few images.  (The fourth item this list held, a mask for cv::FAST, is vo_fast_mask.h, the tenth header: vofm_set_params does for
 * VODET_FAST what this record does for VODET_SHI_TOMASI; each record has no effect under the other detector.)
 */
#ifndef VO_TOPUP_H
#define VO_TOPUP_H

#include "vo_detector.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VOTOP_OFF 0
#define VOTOP_CARRIED 1

typedef struct votop_params {
    int mode;   /* VOTOP_* */
    int radius; /* 0 .. VOCORN_MAX_MIN_DISTANCE */
} votop_params;

/* VOTOP_OFF, radius 5 */
void votop_default_params(votop_params *p);

/* The top-up of the frame loop from now on.  p == NULL: the defaults. */
int votop_set_params(vo_ctx *ctx, const votop_params *p);

/* The record in force. */
int votop_get_params(const vo_ctx *ctx, votop_params *p);

/* The mask plane (h rows of w bytes, mask_stride apart) the last vo_detect_bucket (frame 0) or VO_STAGE_DETECT built for `frame`.
 * VO_ERR_STATE inside the sequence loop, when no masked detection has run on the table as it is configured, and for a frame that
 * did not detect again. */
int votop_get_mask(vo_ctx *ctx, int frame, uint8_t *mask_out, int mask_stride);

#ifdef __cplusplus
}
#endif
#endif /* VO_TOPUP_H */
