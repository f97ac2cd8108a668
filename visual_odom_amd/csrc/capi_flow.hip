// capi_flow.hip -- the two-image tracker of include/vo_flow.h: voflow_track, voflow_feature_tracking (the reference's
// featureTracking(), feature.cpp:64-74) and the throughput mode voflow_batch_*.  One hop of the LK kernel between an arbitrary
// (prev, next) pair with the err output (lk.hip: lk_flow_kernel), deleteUnmatchFeatures on the device (post.hip:
// flow_compact_kernel).  Its device memory comes from the context's Owner at the first voflow_* call: a context that never makes
// one allocates and launches what it always did.
// The calls of include/vo_flow_win.h (vowin_*) are the same host code with a window: every call below takes `win`, voflow_* pass
// 21 (lk_flow_kernel), vowin_* the caller's (lk_flow_win_kernel<win>, refused before anything is launched if there is none).
// The calls of include/vo_flow_flags.h (voflag_*) are the same host code again with cv::calcOpticalFlowPyrLK's flags: voflow_* and
// vowin_* pass 0 and reach the kernels they always reached, anything else is lk_flow_flags_kernel<win> (launch_lk_flow's route).
#include "capi_internal.h"
#include "../../include/vo_flow_flags.h"

namespace {

// the pairs of the synchronous calls, resident behind the batch pairs (d_pairs + max_frames): prev in image slot 0, next in
// slot 1 -- or in slot 2 in a context with rectification maps, where an upload's side is the parity of its slot and both images
// of a mono call are LEFT images
#define VO_FLOW_CONST_PAIRS 2
const vo::Quad VO_FLOW_CONST_PAIR_TABLE[VO_FLOW_CONST_PAIRS] = {{0, 1, 0, 1}, {0, 2, 0, 2}};

int ensure_flow(vo_ctx *c)
{
    vo_ctx::Flow &fl = c->flow;
    if (fl.ready)
        return VO_OK;
    VO_HIP_TRY(c, hipSetDevice(c->device));
    const size_t B = (size_t)c->max_frames, cap = (size_t)c->cap;
    Owner &o = c->own;
    bool ok = o.device(&fl.d_pairs, B + VO_FLOW_CONST_PAIRS);
    ok = ok && o.device(&fl.d_next, B * cap);
    ok = ok && o.device(&fl.d_status, B * cap);
    ok = ok && o.device(&fl.d_err, B * cap);
    ok = ok && o.device(&fl.d_out0, cap);
    ok = ok && o.device(&fl.d_out1, cap);
    ok = ok && o.device(&fl.d_idx, cap);
    ok = ok && o.device(&fl.d_nout, (size_t)1, /*zero*/ true);
    if (!ok) // (what was handed out stays with the Owner and goes with the context; the next call tries again)
        return fail_hip(c, "voflow: device memory for the flow outputs", o.err);
    VO_HIP_TRY(c, hipMemcpy(fl.d_pairs + B, VO_FLOW_CONST_PAIR_TABLE, sizeof(VO_FLOW_CONST_PAIR_TABLE), hipMemcpyHostToDevice));
    fl.h_pairs.assign(B, Quad{0, 0, 0, 0});
    fl.next_set.assign(B, (uint8_t)0);
    fl.ready = true;
    return VO_OK;
}

// Both synchronous calls: two uploads through the pull path (the points ride with the second), two pyramids, one hop, with
// `compact` deleteUnmatchFeatures, one gather into the host-visible result buffer, one synchronisation.  With
// VOFLAG_USE_INITIAL_FLOW the n guesses go to the next-position rows ahead of the hop, one copy on the tracking stream: the pull
// path's staging carries one point list per call, and the call returns behind its one synchronisation whatever memory they lie in.
int flow_sync_call(vo_ctx *c, const char *who, const uint8_t *prev, const uint8_t *next, int w, int h, int stride, const float *pts, int n,
                   int win, int flags, const float *guess, bool want_err, bool compact)
{
    if (c->seq.on)
        return fail(c, VO_ERR_STATE, (std::string(who) + " inside the sequence loop (vo_seq_*)").c_str());
    if (n > c->cap)
        return fail(c, VO_ERR_ARG, (std::string(who) + ": more points than max_pts given to vo_create").c_str());
    if (w < 32 || h < 32 || w > c->max_w || h > c->max_h)
        return fail(c, VO_ERR_ARG, (std::string(who) + ": image size beyond the capacity given to vo_create").c_str());
    if (stride < w * ingest_bpp(c->prm.input_format))
        return fail(c, VO_ERR_ARG, (std::string(who) + ": stride smaller than the width (x bytes per pixel of vo_params.input_format)").c_str());
    int rc = ensure_flow(c);
    if (rc != VO_OK)
        return rc;
    rc = vo_batch_configure(c, 4, w, h, 1);
    if (rc != VO_OK)
        return rc;
    rc = sync_all(c); // a queued run of the batch API may still read the points / write the staging slots
    if (rc != VO_OK)
        return rc;
    vo_ctx::Flow &fl = c->flow;
    // the image slots of the drop-in calls are overwritten: no kept pair, and the batch tables are the caller's to set again
    c->tf_base = -1;
    c->defer.n = 0;
    c->stage_next = 0;
    c->pts_sel = -1;
    c->quads_set = false;
    fl.n_pairs = 0;
    const int k = c->prm.rectify ? 1 : 0, slot1 = VO_FLOW_CONST_PAIR_TABLE[k].r0;
    rc = upload_image(c, 0, prev, stride, hipMemcpyHostToDevice, /*idle*/ true);
    if (rc != VO_OK)
        return rc;
    rc = upload_image(c, slot1, next, stride, hipMemcpyHostToDevice, /*idle*/ true, pts, n); // (+ the points and their count, frame 0)
    if (rc != VO_OK)
        return rc;
    c->h_npts[0] = n;
    c->pts_on_device = false;
    c->max_pts_set = n;
    hipStream_t st = c->sel->stream;
    launch_pyramid_fused(c->d_imgs, slot1 + 1, c->levels, c->lw, c->lh, c->lstride, st); // (slot 1 of a rectifying context: rebuilt as it is)
    std::fill(c->img_stale.begin(), c->img_stale.begin() + slot1 + 1, (uint8_t)0);
    if (flags & VOFLAG_USE_INITIAL_FLOW)
        VO_HIP_TRY(c, hipMemcpyAsync(fl.d_next, guess, sizeof(float2) * (size_t)n, hipMemcpyHostToDevice, st));
    launch_lk_flow(win, flags, c->d_imgs, fl.d_pairs + c->max_frames + k, c->d_pts, c->d_npts, c->cap, n, 1, fl.d_next, fl.d_status,
                   want_err ? fl.d_err : nullptr, lk_params(c), st);
    if (compact)
        launch_flow_compact(c->d_pts, fl.d_next, fl.d_status, c->d_npts, c->cap, fl.d_out0, fl.d_out1, fl.d_idx, fl.d_nout, 1, st);
    FlowGather g;
    g.next = fl.d_next;
    g.out0 = fl.d_out0;
    g.out1 = fl.d_out1;
    g.status = fl.d_status;
    g.err = want_err ? fl.d_err : nullptr;
    g.keep_idx = fl.d_idx;
    g.n_out = fl.d_nout;
    g.n = n;
    g.cap = c->cap;
    g.compact = compact ? 1 : 0;
    launch_flow_gather(g, c->d_gather, st);
    VO_HIP_TRY(c, hipGetLastError());
    VO_HIP_TRY(c, hipStreamSynchronize(st));
    return VO_OK;
}

// the windows with a kernel: odd, 5 .. 21 (vo_flow_win.h says why 23 and above are out) -- launch_lk_flow's precondition,
// checked by every entry point before anything else happens
bool win_ok(int win) { return win >= 5 && win <= 21 && (win & 1); }
int bad_win(vo_ctx *c, const char *who) { return fail(c, VO_ERR_ARG, (std::string(who) + ": win is not an odd number of 5 .. 21").c_str()); }
// the flags with a meaning (vo_flow_flags.h), checked like the window
bool flags_ok(int flags) { return (flags & ~(VOFLAG_USE_INITIAL_FLOW | VOFLAG_GET_MIN_EIGENVALS)) == 0; }
int bad_flags(vo_ctx *c, const char *who)
{
    return fail(c, VO_ERR_ARG, (std::string(who) + ": flags holds a bit other than VOFLAG_USE_INITIAL_FLOW | VOFLAG_GET_MIN_EIGENVALS").c_str());
}

int track(vo_ctx *c, const char *who, const uint8_t *prev, const uint8_t *next, int w, int h, int stride, const float *prev_pts_xy, int n,
          int win, int flags, float *next_pts_xy /* in (the guesses, VOFLAG_USE_INITIAL_FLOW) / out */, uint8_t *status, float *err)
{
    if (!c)
        return VO_ERR_ARG;
    if (!prev || !next || n < 0 || (n > 0 && (!prev_pts_xy || !next_pts_xy || !status)))
        return fail(c, VO_ERR_ARG, (std::string(who) + ": null image / points / output, or n < 0").c_str());
    if (!win_ok(win))
        return bad_win(c, who);
    if (!flags_ok(flags))
        return bad_flags(c, who);
    if (n == 0 && !c->seq.on)
        return VO_OK;
    int rc = flow_sync_call(c, who, prev, next, w, h, stride, prev_pts_xy, n, win, flags, next_pts_xy, err != nullptr, /*compact*/ false);
    if (rc != VO_OK)
        return rc;
    const uint8_t *hb = c->h_gather;
    const FlowGatherLayout L{(size_t)c->cap};
    memcpy(next_pts_xy, hb + L.next(), sizeof(float2) * (size_t)n);
    memcpy(status, hb + L.status(), (size_t)n);
    if (err)
        memcpy(err, hb + L.err(), sizeof(float) * (size_t)n);
    return VO_OK;
}

int feature_tracking(vo_ctx *c, const char *who, const uint8_t *prev, const uint8_t *next, int w, int h, int stride, float *pts0_io, int n,
                     int win, int flags, float *pts1_out /* in (the guesses, VOFLAG_USE_INITIAL_FLOW) / out */, uint8_t *status, float *err,
                     int32_t *keep_idx, int *n_out)
{
    if (!c)
        return VO_ERR_ARG;
    if (!prev || !next || !n_out || n < 0 || (n > 0 && (!pts0_io || !pts1_out || !status)))
        return fail(c, VO_ERR_ARG, (std::string(who) + ": null image / points / output, or n < 0").c_str());
    if (!win_ok(win))
        return bad_win(c, who);
    if (!flags_ok(flags))
        return bad_flags(c, who);
    if (n == 0 && !c->seq.on)
        return VO_OK;
    int rc = flow_sync_call(c, who, prev, next, w, h, stride, pts0_io, n, win, flags, pts1_out, err != nullptr, /*compact*/ true);
    if (rc != VO_OK)
        return rc;
    const uint8_t *hb = c->h_gather;
    const FlowGatherLayout L{(size_t)c->cap};
    int count = peek<int>(hb + L.count);
    count = count < 0 ? 0 : count > n ? n : count;
    if (count > 0) {
        memcpy(pts0_io, hb + L.out0(), sizeof(float2) * (size_t)count);
        memcpy(pts1_out, hb + L.out1(), sizeof(float2) * (size_t)count);
        if (keep_idx)
            memcpy(keep_idx, hb + L.keep_idx(), sizeof(int32_t) * (size_t)count);
    }
    memcpy(status, hb + L.status(), (size_t)n);
    if (err)
        memcpy(err, hb + L.err(), sizeof(float) * (size_t)n);
    *n_out = count;
    return VO_OK;
}

int batch_run(vo_ctx *c, const char *who, int win, int flags)
{
    if (!c)
        return VO_ERR_ARG;
    const std::string me(who);
    if (!win_ok(win))
        return bad_win(c, who);
    if (!flags_ok(flags))
        return bad_flags(c, who);
    if (c->seq.on)
        return fail(c, VO_ERR_STATE, (me + " inside the sequence loop (vo_seq_*)").c_str());
    vo_ctx::Flow &fl = c->flow;
    if (c->n_images == 0)
        return fail(c, VO_ERR_STATE, (me + " before vo_batch_configure").c_str());
    if (!fl.ready || fl.n_pairs == 0 || fl.cfg[0] != c->n_images || fl.cfg[1] != c->w || fl.cfg[2] != c->h || fl.cfg[3] != c->n_frames)
        return fail(c, VO_ERR_STATE, (me + ": no pairs set for this table (voflow_batch_set_pairs after vo_batch_configure)").c_str());
    for (int f = 0; f < fl.n_pairs; f++)
        if (c->img_stale[fl.h_pairs[f].l0] | c->img_stale[fl.h_pairs[f].r0])
            return fail(c, VO_ERR_STATE, (me + ": an image uploaded after its pyramid was last built (run VO_STAGE_PYRAMID over it first)").c_str());
    if (flags & VOFLAG_USE_INITIAL_FLOW)
        for (int f = 0; f < fl.n_pairs; f++)
            if (!fl.next_set[f])
                return fail(c, VO_ERR_STATE, (me + ": VOFLAG_USE_INITIAL_FLOW, and a frame's next positions hold neither a guess "
                                                   "(voflag_batch_set_guess) nor a run's results since voflow_batch_set_pairs").c_str());
    VO_HIP_TRY(c, hipSetDevice(c->device));
    launch_lk_flow(win, flags, c->d_imgs, fl.d_pairs, cur_pts(c), cur_npts(c), c->cap, c->max_pts_set, fl.n_pairs, fl.d_next, fl.d_status,
                   fl.d_err, lk_params(c), c->sel->stream);
    VO_HIP_TRY(c, hipGetLastError());
    std::fill(fl.next_set.begin(), fl.next_set.begin() + fl.n_pairs, (uint8_t)1); // (every frame's rows are a run's results now)
    return VO_OK;
}

} // namespace

extern "C" {

int voflow_track(vo_ctx *c, const uint8_t *prev, const uint8_t *next, int w, int h, int stride, const float *prev_pts_xy, int n,
                 float *next_pts_xy, uint8_t *status, float *err)
{
    return track(c, "voflow_track", prev, next, w, h, stride, prev_pts_xy, n, 21, 0, next_pts_xy, status, err);
}

int voflow_feature_tracking(vo_ctx *c, const uint8_t *prev, const uint8_t *next, int w, int h, int stride, float *pts0_io, int n,
                            float *pts1_out, uint8_t *status, float *err, int32_t *keep_idx, int *n_out)
{
    return feature_tracking(c, "voflow_feature_tracking", prev, next, w, h, stride, pts0_io, n, 21, 0, pts1_out, status, err, keep_idx, n_out);
}

int vowin_track(vo_ctx *c, const uint8_t *prev, const uint8_t *next, int w, int h, int stride, const float *prev_pts_xy, int n, int win,
                float *next_pts_xy, uint8_t *status, float *err)
{
    return track(c, "vowin_track", prev, next, w, h, stride, prev_pts_xy, n, win, 0, next_pts_xy, status, err);
}

int vowin_feature_tracking(vo_ctx *c, const uint8_t *prev, const uint8_t *next, int w, int h, int stride, float *pts0_io, int n, int win,
                           float *pts1_out, uint8_t *status, float *err, int32_t *keep_idx, int *n_out)
{
    return feature_tracking(c, "vowin_feature_tracking", prev, next, w, h, stride, pts0_io, n, win, 0, pts1_out, status, err, keep_idx, n_out);
}

int vowin_batch_run(vo_ctx *c, int win) { return batch_run(c, "vowin_batch_run", win, 0); }

// the deepest level plan_levels gives an image of this size under the context's lk_max_level.  The context is const, as in
// vo_model_bytes: a refusal leaves vo_last_error as it was.
int vowin_max_level(const vo_ctx *c, int w, int h, int *max_level)
{
    if (!c || !max_level || w < 32 || h < 32 || w > c->max_w || h > c->max_h)
        return VO_ERR_ARG;
    *max_level = plan_depth(w, h, c->prm.lk_max_level);
    return VO_OK;
}

int voflow_batch_set_pairs(vo_ctx *c, const int32_t *pairs2, int n_frames)
{
    if (!c)
        return VO_ERR_ARG;
    if (!pairs2 || n_frames < 1 || n_frames > c->max_frames)
        return fail(c, VO_ERR_ARG, "voflow_batch_set_pairs: null pairs / frame count beyond max_frames");
    if (c->seq.on)
        return fail(c, VO_ERR_STATE, "voflow_batch_set_pairs inside the sequence loop (vo_seq_*)");
    if (c->n_images == 0 || n_frames != c->n_frames)
        return fail(c, VO_ERR_STATE, "voflow_batch_set_pairs: configure first / frame count mismatch");
    for (int i = 0; i < 2 * n_frames; i++)
        if (pairs2[i] < 0 || pairs2[i] >= c->n_images)
            return fail(c, VO_ERR_ARG, "voflow_batch_set_pairs: image index out of range");
    int rc = ensure_flow(c);
    if (rc != VO_OK)
        return rc;
    vo_ctx::Flow &fl = c->flow;
    fl.n_pairs = 0;
    std::fill(fl.next_set.begin(), fl.next_set.end(), (uint8_t)0);
    for (int f = 0; f < n_frames; f++)
        fl.h_pairs[f] = Quad{pairs2[2 * f], pairs2[2 * f + 1], pairs2[2 * f], pairs2[2 * f + 1]};
    VO_HIP_TRY(c, hipSetDevice(c->device));
    rc = sync_all(c); // (a queued voflow_batch_run may still read the table)
    if (rc != VO_OK)
        return rc;
    VO_HIP_TRY(c, hipMemcpy(fl.d_pairs, fl.h_pairs.data(), sizeof(Quad) * (size_t)n_frames, hipMemcpyHostToDevice));
    fl.n_pairs = n_frames;
    fl.cfg[0] = c->n_images, fl.cfg[1] = c->w, fl.cfg[2] = c->h, fl.cfg[3] = c->n_frames;
    return VO_OK;
}

int voflag_track(vo_ctx *c, const uint8_t *prev, const uint8_t *next, int w, int h, int stride, const float *prev_pts_xy, int n, int win,
                 int flags, float *next_pts_io, uint8_t *status, float *err)
{
    return track(c, "voflag_track", prev, next, w, h, stride, prev_pts_xy, n, win, flags, next_pts_io, status, err);
}

int voflag_feature_tracking(vo_ctx *c, const uint8_t *prev, const uint8_t *next, int w, int h, int stride, float *pts0_io, int n, int win,
                            int flags, float *pts1_io, uint8_t *status, float *err, int32_t *keep_idx, int *n_out)
{
    return feature_tracking(c, "voflag_feature_tracking", prev, next, w, h, stride, pts0_io, n, win, flags, pts1_io, status, err, keep_idx, n_out);
}

int voflag_batch_run(vo_ctx *c, int win, int flags) { return batch_run(c, "voflag_batch_run", win, flags); }

// the guesses of one frame into the rows the run reads and writes; ordered behind a queued run on the context's stream
int voflag_batch_set_guess(vo_ctx *c, int frame, const float *next_pts_xy, int n)
{
    if (!c)
        return VO_ERR_ARG;
    if (c->seq.on)
        return fail(c, VO_ERR_STATE, "voflag_batch_set_guess inside the sequence loop (vo_seq_*)");
    if (frame < 0 || frame >= c->max_frames || n < 0 || n > c->cap || (n > 0 && !next_pts_xy))
        return fail(c, VO_ERR_ARG, "voflag_batch_set_guess: bad frame / n, or null points");
    vo_ctx::Flow &fl = c->flow;
    if (c->n_images == 0 || !fl.ready || fl.n_pairs == 0 || fl.cfg[0] != c->n_images || fl.cfg[1] != c->w || fl.cfg[2] != c->h ||
        fl.cfg[3] != c->n_frames)
        return fail(c, VO_ERR_STATE, "voflag_batch_set_guess: no pairs set for this table (voflow_batch_set_pairs first)");
    if (frame >= fl.n_pairs)
        return fail(c, VO_ERR_ARG, "voflag_batch_set_guess: frame beyond the pairs set");
    VO_HIP_TRY(c, hipSetDevice(c->device));
    if (n > 0) {
        VO_HIP_TRY(c, hipMemcpyAsync(fl.d_next + (size_t)frame * c->cap, next_pts_xy, sizeof(float2) * (size_t)n, hipMemcpyHostToDevice,
                                     c->sel->stream));
        VO_HIP_TRY(c, hipStreamSynchronize(c->sel->stream)); // (pageable host memory: safe to return from)
    }
    fl.next_set[frame] = 1;
    return VO_OK;
}

int voflow_batch_run(vo_ctx *c) { return batch_run(c, "voflow_batch_run", 21, 0); }

int voflow_batch_get(vo_ctx *c, int frame, float *next_pts_xy, uint8_t *status, float *err, int n)
{
    if (!c)
        return VO_ERR_ARG;
    if (c->seq.on)
        return fail(c, VO_ERR_STATE, "voflow_batch_get inside the sequence loop (vo_seq_*)");
    if (frame < 0 || frame >= c->max_frames || n < 0 || n > c->cap)
        return fail(c, VO_ERR_ARG, "voflow_batch_get: bad frame / n");
    vo_ctx::Flow &fl = c->flow;
    if (!fl.ready || fl.n_pairs == 0)
        return fail(c, VO_ERR_STATE, "voflow_batch_get: no pairs set (voflow_batch_set_pairs, voflow_batch_run first)");
    if (frame >= fl.n_pairs)
        return fail(c, VO_ERR_ARG, "voflow_batch_get: frame beyond the pairs set");
    VO_HIP_TRY(c, hipSetDevice(c->device));
    const size_t o = (size_t)frame * c->cap;
    D2H(next_pts_xy, fl.d_next + o, sizeof(float2) * (size_t)n);
    D2H(status, fl.d_status + o, (size_t)n);
    D2H(err, fl.d_err + o, sizeof(float) * (size_t)n);
    VO_HIP_TRY(c, hipStreamSynchronize(c->sel->stream));
    return VO_OK;
}

} // extern "C"
