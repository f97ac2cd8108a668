/*
 * vo_flow_flags.h -- the two-image tracker of vo_flow.h / vo_flow_win.h with the last argument of cv::calcOpticalFlowPyrLK those
 * calls hard-wire: `flags`.  voflag_track, voflag_feature_tracking and voflag_batch_run are vowin_track, vowin_feature_tracking
 * and vowin_batch_run with OpenCV's two flags, under OpenCV's own values:
 *
 *   VOFLAG_USE_INITIAL_FLOW (4)    the search starts at the caller's guess of the next position, not at the previous position;
 *   VOFLAG_GET_MIN_EIGENVALS (8)   err is the min eigenvalue of the point's structure tensor, not the L1 residual.
 *
 * Everything vo_flow.h and vo_flow_win.h say holds here word for word: the context, the image formats and strides, RECTIFICATION,
 * the KEPT PAIR (none after a synchronous call; the batch tables are to be set again), the ERRORS, the windows (odd, 5 .. 21) and
 * the PYRAMID DEPTH E = vowin_max_level.  In addition: flags == 0 IS the vowin_* call, byte for byte (it runs the same kernel); any
 * bit other than 4 and 8 is VO_ERR_ARG, and nothing is launched.  The result of a call is that of
 *     cv::calcOpticalFlowPyrLK(prev, next, prev_pts, next_pts, status, err, Size(win, win), E,
 *                              TermCriteria(COUNT + EPS, lk_max_count, lk_epsilon), flags, lk_min_eig_threshold)
 * bit for bit.
 *
 * USE_INITIAL_FLOW.  The next-position array is IN/OUT: n guesses in, n results out.  At the deepest level E the search starts at
 * guess * 2^-E (one exact multiply per coordinate); below it at twice the previous level's result, as always.  The template side --
 * prev_pts, its admissibility test, its weights -- does not see the guess.
 *   * A point whose level-0 template window is inadmissible reports status 0 and the propagated position: the guess * 2^-E, doubled
 *     once per level -- the guess itself.
 *   * A guess that is NaN, +-inf, beyond int32 or far outside the image fails at the first cell entry of every level (the rule
 *     vo_hip.h documents for start points: NaN counts as "left of the window", as cvFloor(NaN) = INT_MIN does on x86): status 0,
 *     and the propagated value is its position.
 *   * A guess equal to prev_pts gives the bytes of the flags-0 call.
 * What it buys: a caller who knows roughly where a point went (the previous frame's flow of a carried feature, a disparity prior,
 * an IMU prediction) can track on fewer levels and spends fewer iterations (lk_max_level = 0 with a good guess).
 *
 * GET_MIN_EIGENVALS.  err[i] = (A22 + A11 - sqrt((A11 - A22)^2 + 4 A12^2)) / (2 win^2) of the LEVEL-0 template of point i, in f32
 * with correctly rounded sqrt and divide -- the quantity lk_min_eig_threshold is compared with, and the Shi-Tomasi score of the
 * point at the tracker's own window.  It is written whenever the level-0 template window is admissible, whatever the status ends
 * as: a point rejected for minEig < threshold or for a singular tensor still reports its value.  It is 0 when that window is
 * inadmissible.  As in OpenCV the L1 residual is not computed, and neither is the final in-bounds check that belongs to it --
 * with err == NULL too -- so status is that of an OpenCV call WITHOUT an err vector: a point whose last step left the image keeps
 * status 1.  Positions do not depend on this flag.
 *
 * Both flags together: both rules.
 *
 * THROUGHPUT MODE.  The next-position rows voflow_batch_get reads are the rows a run with USE_INITIAL_FLOW starts from: what
 * voflag_batch_set_guess put there, or what the previous run (voflow_, vowin_ or voflag_batch_run) left -- so a second run with
 * the flag refines the first.  Such a run while a frame's rows hold neither since voflow_batch_set_pairs is VO_ERR_STATE.
 */
#ifndef VO_FLOW_FLAGS_H
#define VO_FLOW_FLAGS_H

#include "vo_flow_win.h"

#define VOFLAG_USE_INITIAL_FLOW 4  /* cv::OPTFLOW_USE_INITIAL_FLOW */
#define VOFLAG_GET_MIN_EIGENVALS 8 /* cv::OPTFLOW_LK_GET_MIN_EIGENVALS */

#ifdef __cplusplus
extern "C" {
#endif

/* vowin_track with flags.  next_pts_io is in/out: with VOFLAG_USE_INITIAL_FLOW the n guesses in; always the n results out. */
int voflag_track(vo_ctx *ctx, const uint8_t *prev, const uint8_t *next, int w, int h, int stride, const float *prev_pts_xy, int n, int win,
                 int flags, float *next_pts_io, uint8_t *status, float *err);

/* vowin_feature_tracking with flags: the call above + deleteUnmatchFeatures over its outputs.  pts1_io: the n guesses in (with
 * VOFLAG_USE_INITIAL_FLOW), the n_out survivors' positions out. */
int voflag_feature_tracking(vo_ctx *ctx, const uint8_t *prev, const uint8_t *next, int w, int h, int stride, float *pts0_io, int n, int win,
                            int flags, float *pts1_io, uint8_t *status, float *err, int32_t *keep_idx, int *n_out);

/* The guesses of one frame of the throughput mode: n points into the first n next-position rows of `frame` (copied before the call
 * returns).  VO_ERR_ARG: frame outside the frames the pairs were set for, n outside 0 .. max_pts, NULL points with n > 0;
 * VO_ERR_STATE: inside vo_seq_*, or no pairs set for the configured table. */
int voflag_batch_set_guess(vo_ctx *ctx, int frame, const float *next_pts_xy, int n);

/* vowin_batch_run with flags; results through voflow_batch_get as before. */
int voflag_batch_run(vo_ctx *ctx, int win, int flags);

#ifdef __cplusplus
}
#endif
#endif /* VO_FLOW_FLAGS_H */
