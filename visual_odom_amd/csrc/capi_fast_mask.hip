// capi_fast_mask.hip -- cv::FAST under a mask (include/vo_fast_mask.h, vofm_*): the checked record in vo_ctx, the mask planes and the
// two corner lists of the frames, the one route every caller takes behind cv::FAST's unmasked list -- discs of the carried points
// (corn_disc_frames_kernel, corners.hip), fast_mask_filter_kernel (fast.hip) -- and the synchronous calls vofm_detect / vofm_replenish,
// which are that route on one frame with the caller's mask, or the discs of the caller's points, in plane 0.
#include "capi_internal.h"
#include "vo_corners_dev.h"

namespace vo_capi {

// One plane of max_w x max_h bytes per frame, 16 bytes apart at least, d_table[f] = plane f, and the two lists.  Growing drains the
// context (a queued run may still read what is given back): never inside a lock-step step.
int fm_ensure(vo_ctx *c, int frames)
{
    vo_ctx::FastMask &t = c->fm;
    if (t.slots >= frames)
        return VO_OK;
    VO_HIP_TRY(c, hipSetDevice(c->device));
    int rc = sync_all(c);
    if (rc != VO_OK)
        return rc;
    Owner &o = c->own;
    (void)o.give_back(&t.d_planes);
    (void)o.give_back(&t.d_table);
    (void)o.give_back(&t.d_raw);
    (void)o.give_back(&t.d_nraw);
    (void)o.give_back(&t.d_filt);
    t.slots = 0;
    t.ran = 0;
    t.plane_stride = ((size_t)c->max_w * c->max_h + 15) & ~(size_t)15;
    const size_t F = (size_t)frames;
    if (!o.device(&t.d_planes, F * t.plane_stride) || !o.device(&t.d_table, F) || !o.device(&t.d_raw, F * c->fcap, /*zero*/ true) ||
        !o.device(&t.d_nraw, F, /*zero*/ true) || !o.device(&t.d_filt, F * c->fcap, /*zero*/ true))
        return fail_hip(c, "vofm: device memory for the mask planes and the corner lists", o.err);
    std::vector<const uint8_t *> tab(F);
    for (size_t f = 0; f < F; f++)
        tab[f] = t.d_planes + f * t.plane_stride;
    VO_HIP_TRY(c, hipMemcpy(t.d_table, tab.data(), sizeof(tab[0]) * tab.size(), hipMemcpyHostToDevice));
    t.slots = frames;
    return VO_OK;
}

static CornTopArgs disc_args(vo_ctx *c, int radius, int max_kept)
{
    vo_ctx::FastMask &t = c->fm;
    CornTopArgs ta;
    ta.feat = c->d_feat;
    ta.fcap = c->fcap;
    ta.n_tracked = c->d_ntracked;
    ta.radius = radius;
    ta.planes = const_cast<uint8_t *const *>(t.d_table);
    ta.plane0 = t.d_planes;
    ta.plane_stride = t.plane_stride;
    ta.max_kept = max_kept;
    return ta;
}

int fm_finish(vo_ctx *c, const int *d_detect, int frames, const float2 *raw, const int *n_raw, hipStream_t stream)
{
    vo_ctx::FastMask &t = c->fm;
    if (t.slots < frames)
        return fail(c, VO_ERR_STATE, "the FAST mask's planes are fewer than the run's frames");
    VO_HIP_TRY(c, launch_corner_disc_frames(d_detect, frames, c->w, c->h, disc_args(c, t.prm.radius, c->dprm.redetect_below - 1), stream));
    launch_fast_mask_filter(raw, n_raw, c->fcap, t.d_table, c->w, d_detect, t.d_filt, c->d_nnew, frames, stream);
    t.ran = c->seq.on ? 0 : frames;
    t.cfg[0] = c->n_images, t.cfg[1] = c->w, t.cfg[2] = c->h;
    return VO_OK;
}

namespace {

// the checks both synchronous calls make before anything touches the device
int check_call(vo_ctx *c, const char *who, int w, float *pts_out, int cap, int *n_out)
{
    if (!n_out || cap < 0 || (cap > 0 && !pts_out))
        return fail(c, VO_ERR_ARG, (std::string(who) + ": null output, or cap < 0").c_str());
    if (w > 4096)
        return fail(c, VO_ERR_ARG, (std::string(who) + ": images up to 4096 pixels wide").c_str());
    if (c->seq.on)
        return fail(c, VO_ERR_STATE, (std::string(who) + " inside the sequence loop (vo_seq_*)").c_str());
    return VO_OK;
}

// image in (vo_fast_detect's set-up), the one-frame buffers, and the frame's list head on the device: n_kept carried points from the
// staging buffer (the caller has put them there), detect = 1
int begin_call(vo_ctx *c, const uint8_t *img, int w, int h, int stride, int n_kept)
{
    int rc = single_image_setup(c, img, w, h, stride, /*plain*/ true); // (cv::FAST's counterpart: never rectified)
    if (rc == VO_OK)
        rc = fm_ensure(c, 1);
    if (rc != VO_OK)
        return rc;
    launch_features_in(c->d_feat_stage, features_in_ages(c->fcap), n_kept, 0, /*detect*/ 1, c->d_feat, c->d_fages, c->fcap, c->d_ntracked, c->d_detect,
                       c->sel->stream);
    c->h_ntracked[0] = n_kept;
    c->h_detect[0] = 1;
    c->detect_uploaded = true;
    c->fm.ran = 0; // (plane 0 no longer holds a run's mask)
    return VO_OK;
}

// cv::FAST into the raw list, the filter under plane 0, and the results
int finish_call(vo_ctx *c, const char *who, int w, int h, int threshold, int nonmax, float *pts_out, int cap, int *n_out)
{
    vo_ctx::FastMask &t = c->fm;
    hipStream_t s = c->sel->stream;
    threshold = threshold < 0 ? 0 : threshold > 255 ? 255 : threshold;
    launch_fast_corners(c->d_imgs, c->quads_cur, c->d_detect, 1, w, h, threshold, nonmax, c->d_nmsmask, c->d_rowcnt, c->d_rowoff, nullptr, t.d_nraw,
                        c->fcap, t.d_raw, s);
    launch_fast_mask_filter(t.d_raw, t.d_nraw, c->fcap, t.d_table, w, c->d_detect, t.d_filt, c->d_nnew, 1, s);
    VO_HIP_TRY(c, hipGetLastError());
    int n_raw = 0, n = 0;
    VO_HIP_TRY(c, hipMemcpyAsync(&n_raw, t.d_nraw, sizeof(int), hipMemcpyDeviceToHost, s));
    VO_HIP_TRY(c, hipMemcpyAsync(&n, c->d_nnew, sizeof(int), hipMemcpyDeviceToHost, s));
    VO_HIP_TRY(c, hipStreamSynchronize(s));
    if (n_raw > c->fcap) { // the filter read a list that is not cv::FAST's
        *n_out = n_raw;
        return fail(c, VO_ERR_OVERFLOW, (std::string(who) + ": more unmasked corners than the context's corner-list capacity (max(4 x max_pts, 16384, "
                                                            "max_w x max_h / 16)): nothing was written, *n_out is the unmasked count")
                                            .c_str());
    }
    const int k = n < cap ? n : cap;
    if (k > 0)
        VO_HIP_TRY(c, hipMemcpy(pts_out, t.d_filt, sizeof(float2) * (size_t)k, hipMemcpyDeviceToHost));
    *n_out = n;
    return VO_OK;
}

} // namespace

} // namespace vo_capi

extern "C" {

int vofm_detect(vo_ctx *c, const uint8_t *img, int w, int h, int stride, int threshold, int nonmax, const uint8_t *mask, int mask_stride, float *pts_out,
                int cap, int *n_out)
{
    if (!c)
        return VO_ERR_ARG;
    if (!mask) {
        if (mask_stride != 0)
            return fail(c, VO_ERR_ARG, "vofm_detect: a mask stride without a mask");
        return vo_fast_detect(c, img, w, h, stride, threshold, nonmax, pts_out, cap, n_out);
    }
    if (mask_stride < w)
        return fail(c, VO_ERR_ARG, "vofm_detect: mask stride smaller than the width");
    int rc = check_call(c, "vofm_detect", w, pts_out, cap, n_out);
    if (rc == VO_OK)
        rc = begin_call(c, img, w, h, stride, 0);
    if (rc != VO_OK)
        return rc;
    VO_HIP_TRY(c, hipMemcpy2DAsync(c->fm.d_planes, (size_t)w, mask, (size_t)mask_stride, (size_t)w, (size_t)h, hipMemcpyHostToDevice, c->sel->stream));
    return finish_call(c, "vofm_detect", w, h, threshold, nonmax, pts_out, cap, n_out); // (it waits for the stream)
}

int vofm_replenish(vo_ctx *c, const uint8_t *img, int w, int h, int stride, int threshold, int nonmax, const float *kept_xy, int n_kept, int radius,
                   float *pts_out, int cap, int *n_out)
{
    if (!c)
        return VO_ERR_ARG;
    if (n_kept < 0 || n_kept > c->cap || (n_kept > 0 && !kept_xy))
        return fail(c, VO_ERR_ARG, "vofm_replenish: n_kept outside 0 .. max_pts, or null points");
    if (radius < 0 || radius > VOCORN_MAX_MIN_DISTANCE)
        return fail(c, VO_ERR_ARG, "vofm_replenish: radius outside 0 .. VOCORN_MAX_MIN_DISTANCE (256)");
    int rc = check_call(c, "vofm_replenish", w, pts_out, cap, n_out);
    if (rc != VO_OK)
        return rc;
    // (the staging buffer is read by features_in_kernel on the stream; the set-up inside begin_call drains the context first)
    rc = sync_all(c);
    if (rc != VO_OK)
        return rc;
    if (n_kept > 0)
        memcpy(c->h_feat_stage, kept_xy, sizeof(float2) * (size_t)n_kept);
    rc = begin_call(c, img, w, h, stride, n_kept);
    if (rc != VO_OK)
        return rc;
    VO_HIP_TRY(c, launch_corner_disc_frames(c->d_detect, 1, w, h, disc_args(c, radius, n_kept), c->sel->stream));
    return finish_call(c, "vofm_replenish", w, h, threshold, nonmax, pts_out, cap, n_out);
}

void vofm_default_params(vofm_params *p)
{
    if (!p)
        return;
    p->mode = VOFM_OFF;
    p->radius = 5;
}

int vofm_set_params(vo_ctx *c, const vofm_params *p)
{
    if (!c)
        return VO_ERR_ARG;
    vofm_params d;
    if (p)
        d = *p;
    else
        vofm_default_params(&d);
    if (d.mode != VOFM_OFF && d.mode != VOFM_CARRIED)
        return fail(c, VO_ERR_ARG, "vofm_set_params: unknown mode (VOFM_OFF, VOFM_CARRIED)");
    if (d.radius < 0 || d.radius > VOCORN_MAX_MIN_DISTANCE)
        return fail(c, VO_ERR_ARG, "vofm_set_params: radius outside 0 .. VOCORN_MAX_MIN_DISTANCE (256)");
    if (c->seq.on)
        return fail(c, VO_ERR_STATE, "vofm_set_params inside the sequence loop (vo_seq_*): the loop took its mask planes and probed its "
                                     "schedule with the record in force");
    c->fm.prm = d;
    c->fm.ran = 0;
    return VO_OK;
}

int vofm_get_params(const vo_ctx *c, vofm_params *p)
{
    if (!c || !p)
        return VO_ERR_ARG;
    *p = c->fm.prm;
    return VO_OK;
}

int vofm_get_mask(vo_ctx *c, int frame, uint8_t *mask_out, int mask_stride)
{
    if (!c)
        return VO_ERR_ARG;
    if (!mask_out || mask_stride < c->w)
        return fail(c, VO_ERR_ARG, "vofm_get_mask: null output, or a mask stride smaller than the width");
    if (c->seq.on)
        return fail(c, VO_ERR_STATE, "vofm_get_mask inside the sequence loop (vo_seq_*)");
    const vo_ctx::FastMask &t = c->fm;
    if (t.ran == 0 || t.cfg[0] != c->n_images || t.cfg[1] != c->w || t.cfg[2] != c->h)
        return fail(c, VO_ERR_STATE, "vofm_get_mask: no masked detection on the table as it is configured now");
    if (frame < 0 || frame >= t.ran)
        return fail(c, VO_ERR_ARG, "vofm_get_mask: frame outside the latest masked detection");
    if (!c->h_detect[(size_t)frame])
        return fail(c, VO_ERR_STATE, "vofm_get_mask: this frame did not detect again");
    VO_HIP_TRY(c, hipSetDevice(c->device));
    VO_HIP_TRY(c, hipMemcpy2DAsync(mask_out, (size_t)mask_stride, t.d_planes + (size_t)frame * t.plane_stride, (size_t)c->w, (size_t)c->w, (size_t)c->h,
                                   hipMemcpyDeviceToHost, c->sel->stream));
    VO_HIP_TRY(c, hipStreamSynchronize(c->sel->stream));
    return VO_OK;
}

} // extern "C"
