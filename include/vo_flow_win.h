/*
 * vo_flow_win.h -- the two-image tracker of vo_flow.h with the one argument of cv::calcOpticalFlowPyrLK that vo_params does not
 * carry: winSize.  vowin_track, vowin_feature_tracking and vowin_batch_run are voflow_track, voflow_feature_tracking and
 * voflow_batch_run with a square window `win` x `win`, win odd, 5 .. 21.
 *
 * Everything vo_flow.h says holds here word for word: the context (the same vo_ctx, one per host thread per GPU), the image
 * formats and strides (vo_params.input_format), RECTIFICATION (the synchronous calls remap both images through the LEFT maps),
 * the KEPT PAIR (none after a synchronous call; the batch tables are to be set again), the outputs and the ERRORS (vowin_max_level
 * apart, see there).  In addition: win even, below 5 or above 21 is VO_ERR_ARG, and nothing is launched.
 *
 * RESULTS, bit for bit those of OpenCV's CPU tracker with an err vector requested and winSize = Size(win, win):
 *   err = sum over the win x win window of |J(final position) - I| / (32 * win * win)
 * of a point with status 1, 0 of any other; the admissibility tests are the +-win ones and minEigThreshold applies to
 * minEig / (2 * win * win), as in OpenCV.  win = 21 runs the kernel of the voflow_* call and gives its bits.
 *
 * PYRAMID DEPTH.  A windowed call tracks on the pyramid levels the context builds for every call: levels 0 .. E, where E is the
 * largest index not above lk_max_level whose level is still larger than 21 pixels both ways -- the levels a 21 x 21 call uses,
 * whatever `win` is.  OpenCV stops at winSize instead, so on a small image and with a small window a calcOpticalFlowPyrLK(...,
 * Size(win, win), lk_max_level, ...) would go deeper than this library does.  The result of a call here is therefore that of
 *     cv::calcOpticalFlowPyrLK(prev, next, prev_pts, next_pts, status, err, Size(win, win), E,
 *                              TermCriteria(COUNT + EPS, lk_max_count, lk_epsilon), 0, lk_min_eig_threshold)
 * (every level up to E is larger than 21 >= win, so OpenCV builds all of them), and vowin_max_level returns E for an image size,
 * so that a caller can make that very call.  On 1241 x 376, E = lk_max_level for every lk_max_level <= 4 and the call is OpenCV's
 * own; on 480 x 160 with lk_max_level 3, E = 2; on 96 x 64 with lk_max_level 3, E = 1.
 *
 * WHY NOT 23 AND ABOVE.  Every pyramid level is stored with a border of 24 rows above and below and 32 / at least 24 columns left
 * and right, which is what lets a window the reference admits (corner down to -win, up to w - 1) read real memory without a
 * border path.  Every kernel of the library shares that layout; a wider window needs wider borders, i.e. another layout for all
 * of them.  Even and non-square windows are not built.
 */
#ifndef VO_FLOW_WIN_H
#define VO_FLOW_WIN_H

#include "vo_flow.h"

#ifdef __cplusplus
extern "C" {
#endif

/* voflow_track with winSize = Size(win, win) and maxLevel = E (see PYRAMID DEPTH). */
int vowin_track(vo_ctx *ctx, const uint8_t *prev, const uint8_t *next, int w, int h, int stride, const float *prev_pts_xy, int n, int win,
                float *next_pts_xy, uint8_t *status, float *err);

/* voflow_feature_tracking likewise: the call above + deleteUnmatchFeatures. */
int vowin_feature_tracking(vo_ctx *ctx, const uint8_t *prev, const uint8_t *next, int w, int h, int stride, float *pts0_io, int n, int win,
                           float *pts1_out, uint8_t *status, float *err, int32_t *keep_idx, int *n_out);

/* voflow_batch_run likewise, on the table and the pairs of voflow_batch_set_pairs; results through voflow_batch_get. */
int vowin_batch_run(vo_ctx *ctx, int win);

/* E of an image of w x h under the context's lk_max_level (32 <= w, h <= the capacity given to vo_create; no GPU work).  The
 * one exception to the ERRORS of vo_flow.h: the context is const, so a refusal (VO_ERR_ARG: NULL context or output, a size
 * outside that range) leaves vo_last_error() as it was. */
int vowin_max_level(const vo_ctx *ctx, int w, int h, int *max_level);

#ifdef __cplusplus
}
#endif
#endif /* VO_FLOW_WIN_H */
