// capi_dropin.hip -- the synchronous drop-in calls (host buffers in, host buffers out): vo_circular_match, vo_triangulate,
// vo_pnp_ransac, vo_fast_detect, vo_detect_bucket, vo_integrate_odometry, vo_track_frame.
#include "capi_internal.h"

namespace vo_capi {

/* ---------------------------------- drop-in calls ---------------------------------------- */

// The inputs of a single-frame drop-in call on their way to the device WITHOUT a synchronisation in between (round 5): one
// sync_all up front (idle streams: a few microseconds; after it every staging buffer is free and nothing reads the points),
// then four kernels that pull the images out of the pinned staging slots over PCIe (pyramid.hip, launch_pull_image), the last of
// them the points and their count too, all queued on the tracking stream -- the caller's run_stages queues its kernels behind
// them while the pixels are still crossing PCIe.  Round 4 went through vo_batch_set_points here: sync_all + a pageable copy +
// a stream synchronisation, i.e. the host waited for the four uploads (~80 us for KITTI) before it launched anything (108 +
// 21 us of the call, profiles/r04_experiments.md section 7).
int single_frame_setup(vo_ctx *c, const uint8_t *l0, const uint8_t *r0, const uint8_t *l1,
                              const uint8_t *r1, int w, int h, int stride, const float *pts, int n, bool defer_t1)
{
    // no t0 images: the t0 pair is the pair the previous call received as t1 (the reference's loop keeps it the same way,
    // main.cpp:157-158) -- it is on the device with its pyramids, two images cross the link instead of four
    const bool keep = !l0 && !r0;
    if ((!keep && (!l0 || !r0)) || !l1 || !r1 || n < 0 || (n > 0 && !pts))
        return fail(c, VO_ERR_ARG, "null image / points");
    if (n > c->cap)
        return fail(c, VO_ERR_ARG, "more points than max_pts given to vo_create");
    if (stride < w * ingest_bpp(c->prm.input_format)) // (before anything changes: a refused call leaves the kept pair as it is)
        return fail(c, VO_ERR_ARG, "stride smaller than the width (x bytes per pixel of vo_params.input_format)");
    if (keep && !have_kept_pair(c, w, h))
        return fail(c, VO_ERR_STATE, "no t0 images given, and the context does not hold the t1 pair of a previous call of this "
                                     "size (first call, another size, or the batch / sequence API used the images since)");
    int rc = vo_batch_configure(c, 4, w, h, 1);
    if (rc != VO_OK)
        return rc;
    rc = sync_all(c); // a queued run of the batch API may still read the points / write the staging slots
    if (rc != VO_OK)
        return rc;
    static_assert(VO_STAGE_SLOTS >= 4, "one staging slot per image of the call");
    VO_HOST_STAMP(1);
    c->stage_next = 0;
    c->defer.n = 0;
    const int t0 = keep ? c->tf_base : 0, t1 = t0 ^ 2; // image slots of the two pairs
    const uint8_t *imgs[4] = {l0, r0, l1, r1};
    use_const_quad(c, t0 == 0 ? 0 : 1);
    c->tf_base = -1; // (until every image of the call is on its way)
    // one frame: the call's points replace the whole current set, also the bucketed set a VO_STAGE_DETECT run left
    // current (nothing reads that one any more: sync_all above)
    c->pts_sel = -1;
    // Round 6, on the kept pair: hop 0 of the chain (l0 -> r0) reads the t0 pair only, which is on the device with its
    // pyramids -- so only the points go now (a pull of their own) and the t1 pair is DEFERRED to run_stages, which launches
    // hop 0 first and sends the pair on the filter stream beside it (vo_ctx::defer): 0.64 -> 0.61 ms per call at 2 039 points,
    // 0.60 -> 0.58 at 340 (gpurun_out/r6_split1).  Not with four images: two chain launches end on their slowest feature twice
    // (hop 0 alone 74 - 82 us, hops 1 .. 3 172 - 190, the whole chain 200 - 236) and the t0 pyramids become a launch set of their
    // own (27 us) -- measured 0.68 -> 0.70 ms, so four images go the way they always went.
    // (developer build: VO_SYNC_SPLIT=0 is the A/B partner; the split chain runs lk_hops_kernel, so VO_LK_PAIR=1 keeps to one launch)
    const bool split = defer_t1 && keep && dev_knob("VO_SYNC_SPLIT", 1) != 0 && dev_knob("VO_LK_PAIR", 0) != 1;
    for (int i = keep ? 2 : 0; i < (split ? 2 : 4); i++) { // the points travel with the last image
        rc = upload_image(c, (i < 2 ? t0 : t1) + (i & 1), imgs[i], stride, hipMemcpyHostToDevice, /*idle*/ true, pts, i == 3 ? n : -1);
        if (rc != VO_OK)
            return rc;
        VO_HOST_STAMP(2 + i);
    }
    if (split) {
        if (n > 0)
            memcpy(c->h_pts_stage, pts, sizeof(float2) * (size_t)n);
        launch_pull_image(nullptr, nullptr, 0, c->sel->stream, c->d_pts_stage, c->d_pts, n, c->d_npts);
        VO_HIP_TRY(c, hipGetLastError());
        c->defer.img[0] = l1;
        c->defer.img[1] = r1;
        c->defer.first = t1;
        c->defer.stride = stride;
        c->defer.n = 2;
        c->img_stale[t1] = c->img_stale[t1 + 1] = 1; // (what is in those slots is not this call's pair until run_stages has sent it)
    }
    if (keep) {
        c->pyr_first = t1; // (vo_batch_configure above restored "every pyramid")
        c->pyr_count = 2;
    }
    c->tf_base = t1;
    c->tf_gen++; // a new kept pair (vo_kept_pair_id)
    c->h_npts[0] = n;
    c->pts_on_device = false;
    c->max_pts_set = n;
    VO_HOST_STAMP(6);
    return VO_OK;
}

} // namespace vo_capi

extern "C" {

int vo_circular_match(vo_ctx *c, const uint8_t *l0, const uint8_t *r0, const uint8_t *l1, const uint8_t *r1,
                      int w, int h, int stride, const float *pts, int n, float *out_l0, float *out_r0,
                      float *out_r1, float *out_l1, float *out_l0_ret, uint8_t *status4, int32_t *keep_idx,
                      int *n_out, int apply_consistency)
{
    if (!c || !n_out)
        return VO_ERR_ARG;
    DeferGuard guard{c};
    int rc = single_frame_setup(c, l0, r0, l1, r1, w, h, stride, pts, n, /*defer_t1*/ true);
    if (rc != VO_OK)
        return rc;
    // a synchronous call: every stage on the tracking stream (run_stages, `serial`), then ONE kernel that gathers whatever
    // the caller asked for into the host-visible result buffer and one synchronisation (round 5: the batch getters cost this
    // call ten copies and five synchronisations, ~0.17 of its 0.57 ms)
    rc = run_stages_auto(c, VO_STAGE_PYRAMID | VO_STAGE_LK | VO_STAGE_FILTER, false, nullptr, /*sync_call*/ true);
    if (rc != VO_OK)
        return rc;
    const vo_ctx::PoseBufs &pb = c->pb[c->last];
    CircGather g;
    g.outA = c->d_outA;
    g.idxA = c->d_idxA;
    g.nA = c->d_nA;
    g.outB = pb.outB;
    g.idxB = pb.idxB;
    g.nB = pb.nB;
    g.trk = c->d_trk2[c->trk_last];
    g.status = c->d_status2[c->trk_last];
    g.n = status4 ? n : 0;
    g.cap = c->cap;
    g.consistency = apply_consistency ? 1 : 0;
    if (!c->last_run_serial) { // (a run on the batch mode's streams: the filter ran on its own stream and this call has no
                               // pose stage whose event would order the gather behind it -- ADVICE r05)
        rc = sync_all(c);
        if (rc != VO_OK)
            return rc;
    }
    launch_circ_gather(g, c->d_gather, c->sel->stream); // (fits the buffer of the frame gather: vo_kernels.h, CircGatherLayout)
    VO_HIP_TRY(c, hipGetLastError());
    VO_HIP_TRY(c, hipStreamSynchronize(c->sel->stream));
    const uint8_t *hb = c->h_gather;
    const CircGatherLayout L{(size_t)c->cap};
    const int count = peek<int>(hb + L.count);
    float *outs[5] = {out_l0, out_r0, out_r1, out_l1, out_l0_ret};
    for (int k = 0; k < 5; k++)
        if (outs[k] && count > 0)
            memcpy(outs[k], hb + L.row(k), (size_t)count * sizeof(float2));
    if (keep_idx && count > 0)
        memcpy(keep_idx, hb + L.keep_idx(), (size_t)count * sizeof(int32_t));
    if (status4 && n > 0)
        for (int hop = 0; hop < 4; hop++) // [4][n] for the caller
            memcpy(status4 + (size_t)hop * n, hb + L.status(hop), (size_t)n);
    *n_out = count;
    return VO_OK;
}

int vo_triangulate(vo_ctx *c, const float *P_l, const float *P_r, const float *pl, const float *pr, int n,
                   float *xyz_out)
{
    if (!c || !P_l || !P_r || n < 0 || (n > 0 && (!pl || !pr || !xyz_out)))
        return VO_ERR_ARG;
    if (n > c->cap)
        return fail(c, VO_ERR_ARG, "more points than max_pts given to vo_create");
    if (n == 0)
        return VO_OK;
    int rc = vo_batch_set_projection(c, P_l, P_r);
    if (rc != VO_OK)
        return rc;
    rc = sync_all(c);
    if (rc != VO_OK)
        return rc;
    // frame 0, stage-B rows 0 (left) and 1 (right); the points in and the result out through page-locked memory the kernels
    // address (words_in_kernel / words_out_kernel, post.hip): one synchronisation, no copy call
    vo_ctx::PoseBufs &pb = c->pb[c->last];
    memcpy(c->h_feat_stage, pl, sizeof(float2) * (size_t)n);
    memcpy(c->h_feat_stage + sizeof(float2) * (size_t)n, pr, sizeof(float2) * (size_t)n);
    launch_words_in(c->d_feat_stage, 2 * n, pb.outB, 2 * n, pb.outB + c->cap, pb.nB, n, c->sel->stream);
    launch_triangulate(c->d_P, c->d_P + 12, pb.outB, pb.outB + c->cap, (size_t)4 * c->cap, pb.nB, c->cap, n, 1,
                       pb.xyz, c->sel->stream);
    launch_words_out(pb.xyz, 3 * n, c->d_gather, c->sel->stream);
    VO_HIP_TRY(c, hipGetLastError());
    VO_HIP_TRY(c, hipStreamSynchronize(c->sel->stream));
    memcpy(xyz_out, c->h_gather, sizeof(float) * 3 * (size_t)n);
    return VO_OK;
}

int vo_pnp_ransac(vo_ctx *c, const float *xyz, const float *uv, int n, const float *K, double *rvec_io,
                  double *tvec_io, double *R_out, int32_t *inliers, int *n_inliers)
{
    if (!c || !K || n < 0 || (n > 0 && (!xyz || !uv)))
        return VO_ERR_ARG;
    if (n > c->cap)
        return fail(c, VO_ERR_ARG, "more points than max_pts given to vo_create");
    int rcs = sync_all(c);
    if (rcs != VO_OK)
        return rcs;
    vo_ctx::PoseBufs &pb = c->pb[c->last];
    const PnpParams pp = pnp_params(c, K);
    // the correspondences in and the pose out through page-locked memory the kernels address (the staging buffer holds
    // 12 bytes x 4 max_pts or more, a correspondence is 20): one synchronisation per call, no copy call
    if (n > 0) {
        memcpy(c->h_feat_stage, xyz, sizeof(float) * 3 * (size_t)n);
        memcpy(c->h_feat_stage + sizeof(float) * 3 * (size_t)n, uv, sizeof(float2) * (size_t)n);
    }
    launch_words_in(c->d_feat_stage, 3 * n, pb.xyz, 2 * n, pb.outB + 2 * (size_t)c->cap, pb.nB, n, c->sel->stream);
    if (c->n_frames < 1)
        c->n_frames = 1;
    launch_pnp(pb.xyz, pb.outB + 2 * (size_t)c->cap, (size_t)4 * c->cap, pb.nB, c->cap, 1, pp, pb.subsets,
               pb.models, pb.counts, pb.rstate, pb.inliers, pb.results, standalone_waves(c), c->sel->stream, pb.epnp_ws, 1, pb.epnp_gws, pb.rest_ws);
    FrameGather g = {};
    g.nA = g.nB = pb.nB;
    g.inliers = pb.inliers;
    g.result = pb.results;
    g.cap = c->cap;
    g.pose_only = 1;
    launch_frame_gather(g, c->d_gather, c->sel->stream);
    VO_HIP_TRY(c, hipGetLastError());
    VO_HIP_TRY(c, hipStreamSynchronize(c->sel->stream));
    const FrameGatherLayout L{(size_t)c->cap};
    const PnpResult r = peek<PnpResult>(c->h_gather + L.pnp);
    (void)deliver_pose(c, r, nullptr, rvec_io, tvec_io, R_out, /*pnp_rotation*/ true, /*io_pose*/ true); // (R = Rodrigues(rvec) whatever vo_params.mono_rotation says)
    const int ninl = r.n_inliers < c->cap ? r.n_inliers : c->cap;
    if (inliers && ninl > 0)
        memcpy(inliers, c->h_gather + L.inliers(), sizeof(int32_t) * (size_t)ninl);
    if (n_inliers)
        *n_inliers = r.n_inliers;
    if (r.status < 0)
        return fail_too_few_pnp(c);
    return r.status == 1 ? VO_OK : VO_NO_MODEL;
}

} // extern "C"

namespace vo_capi {

// one image as a 1-frame batch whose quad points at image 0 four times
// img == nullptr: the LEFT image of the t1 pair of the previous vo_track_frame / vo_circular_match (what the reference's
// loop detects on next, visualOdometry.cpp:95-108 on imageLeft_t0 = the previous imageLeft_t1) -- nothing is uploaded.
// An image that is given goes to the slot pair that does not hold that t1 pair, which stays valid.
int single_image_setup(vo_ctx *c, const uint8_t *img, int w, int h, int stride, bool plain)
{
    if (img && c && stride < w * ingest_bpp(c->prm.input_format))
        return fail(c, VO_ERR_ARG, "stride smaller than the width (x bytes per pixel of vo_params.input_format)");
    if (!img && !have_kept_pair(c, w, h))
        return fail(c, VO_ERR_STATE, "no image given, and the context does not hold the t1 pair of a previous vo_track_frame "
                                     "of this size");
    int rc = vo_batch_configure(c, 4, w, h, 1);
    if (rc != VO_OK)
        return rc;
    rc = sync_all(c); // a queued run of the batch API may still read the feature lists / the staging slots
    if (rc != VO_OK)
        return rc;
    if (!img) {
        use_const_quad(c, c->tf_base == 0 ? 2 : 3);
        return VO_OK;
    }
    const int slot = c->tf_base == 0 ? 2 : 0;
    const int keep = c->tf_base; // (upload_image itself does not touch it; the batch API's wrappers do)
    c->stage_next = 0;           // (drained above: every staging slot is free, the GPU pulls the image itself)
    rc = upload_image(c, slot, img, stride, hipMemcpyHostToDevice, /*idle*/ true, nullptr, -1, nullptr, plain);
    c->tf_base = rc == VO_OK ? keep : -1;
    if (rc != VO_OK)
        return rc;
    use_const_quad(c, slot == 0 ? 2 : 3);
    return VO_OK;
}

} // namespace vo_capi

extern "C" {

int vo_fast_detect(vo_ctx *c, const uint8_t *img, int w, int h, int stride, int threshold, int nonmax,
                   float *pts_out, int cap, int *n_out)
{
    if (!c || !n_out || cap < 0 || (cap > 0 && !pts_out))
        return VO_ERR_ARG;
    if (w > 4096)
        return fail(c, VO_ERR_ARG, "vo_fast_detect: images up to 4096 pixels wide");
    int rc = single_image_setup(c, img, w, h, stride, /*plain*/ true); // (cv::FAST's counterpart: never rectified)
    if (rc != VO_OK)
        return rc;
    // (no copy call: the flags by features_in_kernel, the corners and their count back through page-locked memory, one
    // synchronisation -- see vo_detect_bucket)
    launch_features_in(c->d_feat_stage, 0, 0, 0, /*detect*/ 1, c->d_feat, c->d_fages, c->fcap, c->d_ntracked, c->d_detect, c->sel->stream);
    c->h_ntracked[0] = 0;
    c->h_detect[0] = 1;
    c->detect_uploaded = true;
    threshold = threshold < 0 ? 0 : threshold > 255 ? 255 : threshold;
    launch_detect_bucket(c->d_imgs, c->quads_cur, c->d_detect, 1, w, h, threshold, nonmax, c->d_nmsmask, c->d_rowcnt, c->d_rowoff,
                         c->d_ntracked, c->d_nnew, c->fcap, c->d_feat, c->d_fages, /*bucket_size*/ 0, 1, nullptr,
                         nullptr, nullptr, 0, nullptr, nullptr, c->sel->stream);
    launch_features_out(c->d_feat, c->d_fages, c->d_nnew, c->d_overflow, c->fcap, c->d_feat_stage, c->sel->stream);
    VO_HIP_TRY(c, hipGetLastError());
    VO_HIP_TRY(c, hipStreamSynchronize(c->sel->stream));
    const int n = peek<int>(c->h_feat_stage + FeaturesOutLayout::count);
    int k = n < cap ? n : cap;
    k = k < c->fcap ? k : c->fcap;
    if (k > 0)
        memcpy(pts_out, c->h_feat_stage + FeaturesOutLayout::pts, sizeof(float2) * (size_t)k);
    *n_out = n;
    if (n > c->fcap && cap > c->fcap) // the caller's buffer would have held them, the context's corner list does not
        return fail(c, VO_ERR_OVERFLOW, "vo_fast_detect: more corners than the context's corner-list capacity "
                                        "(max(4 x max_pts, 16384, max_w x max_h / 16)): only that many were written");
    return VO_OK;
}

int vo_detect_bucket(vo_ctx *c, const uint8_t *img, int w, int h, int stride, const vo_detect_params *dp,
                     float *pts_io, int *n_pts, int32_t *ages_io, int *n_ages, int cap)
{
    if (!c || !n_pts || !n_ages || !pts_io || !ages_io || cap < 1 || *n_pts > cap || *n_ages > cap) // (the arrays hold cap entries)
        return VO_ERR_ARG;
    const int np = *n_pts, na = *n_ages;
    if (np < 0 || na < np || na > c->fcap)
        return fail(c, VO_ERR_ARG, "vo_detect_bucket: bad counts (need 0 <= n_pts <= n_ages <= capacity)");
    int rc = single_image_setup(c, img, w, h, stride);
    if (rc != VO_OK)
        return rc;
    const vo_detect_params saved = c->dprm;
    rc = vo_batch_set_detect_params(c, dp);
    if (rc != VO_OK)
        return rc;
    // The carried set in and the bucketed set out through page-locked memory the kernels address themselves, ONE
    // synchronisation per call (round 5; the batch API's setters and getters cost this call seven copies and five
    // synchronisations, 0.15 of its 0.18 ms on an idle GPU).  single_image_setup has drained the context.
    if (np > 0)
        memcpy(c->h_feat_stage, pts_io, sizeof(float2) * (size_t)np);
    const size_t ages_off = features_in_ages(c->fcap);
    if (na > 0)
        memcpy(c->h_feat_stage + ages_off, ages_io, sizeof(int32_t) * (size_t)na);
    const int detect = np < c->dprm.redetect_below ? 1 : 0; // appendNewFeatures only then (visualOdometry.cpp:95)
    launch_features_in(c->d_feat_stage, ages_off, np, na, detect, c->d_feat, c->d_fages, c->fcap, c->d_ntracked, c->d_detect,
                       c->sel->stream);
    c->h_ntracked[0] = np;
    c->h_detect[0] = detect; // (what run_stages would upload: it finds the flag on the device already)
    c->detect_uploaded = true;
    rc = run_stages(c, VO_STAGE_DETECT, false);
    c->dprm = saved;
    if (rc != VO_OK)
        return rc;
    launch_features_out(cur_pts(c), cur_ages(c), cur_npts(c), c->d_overflow, c->cap, c->d_gather, c->sel->stream);
    VO_HIP_TRY(c, hipGetLastError());
    VO_HIP_TRY(c, hipStreamSynchronize(c->sel->stream));
    const FeaturesOutLayout L{(size_t)c->cap};
    const int k = peek<int>(c->h_gather + L.count), ovf = peek<int>(c->h_gather + L.overflow);
    // (include/vo_detector.h) under Shi-Tomasi the corner list is the select pass's and holds at most the capacity: bit 0 can only
    // mean that the CANDIDATES did not fit, and then no corner was selected at all -- nothing is written
    if (shi_tomasi(c) && (ovf & 1))
        return fail(c, VO_ERR_OVERFLOW, "vo_detect_bucket: more goodFeaturesToTrack candidates than the context's corner-list capacity "
                                        "(max(4 x max_pts, 16384, max_w x max_h / 16)): nothing was written");
    // (include/vo_fast_mask.h) under cv::FAST's mask the filter read a truncated unmasked list: nothing is written either
    if (fastmask_on(c) && (ovf & 1))
        return fail(c, VO_ERR_OVERFLOW, "vo_detect_bucket: more unmasked FAST corners than the context's corner-list capacity "
                                        "(max(4 x max_pts, 16384, max_w x max_h / 16)): nothing was written");
    if (k > cap)
        return fail(c, VO_ERR_ARG, "vo_detect_bucket: bucketed set larger than the caller's capacity");
    const int kc = k < c->cap ? k : c->cap;
    memcpy(pts_io, c->h_gather + L.pts, sizeof(float2) * (size_t)kc);
    memcpy(ages_io, c->h_gather + L.ages(), sizeof(int32_t) * (size_t)kc);
    *n_pts = k;
    *n_ages = k;
    return ovf ? fail_overflow(c, ovf) : VO_OK;
}

int vo_integrate_odometry(double *pose, const double *R, const double *t, float *euler_out)
{
    if (!pose || !R || !t)
        return VO_ERR_ARG;
    return integrate_odometry(pose, R, t, euler_out); // vo_integrate.h: the code the sequence loop runs on the device
}

int vo_track_frame(vo_ctx *c, const uint8_t *l0, const uint8_t *r0, const uint8_t *l1, const uint8_t *r1, int w,
                   int h, int stride, const float *pts, int n, const float *P_l, const float *P_r,
                   float *out_l0, float *out_r0, float *out_l1, float *out_r1, float *xyz_out,
                   int32_t *keep_idx, int *n_out, int32_t *keep_idx_circ, int *n_circ, double *rvec_io,
                   double *tvec_io, double *R_out, int32_t *inliers, int *n_inliers)
{
    if (!c || !P_l || !P_r)
        return VO_ERR_ARG;
    VO_HOST_STAMP(0);
    DeferGuard guard{c};
    int rc = single_frame_setup(c, l0, r0, l1, r1, w, h, stride, pts, n, /*defer_t1*/ true);
    if (rc != VO_OK)
        return rc;
    rc = vo_batch_set_projection(c, P_l, P_r);
    if (rc != VO_OK)
        return rc;
    rc = run_stages_auto(c, VO_STAGE_ALL, false, nullptr, /*sync_call*/ true);
    if (rc != VO_OK)
        return rc;
    VO_HOST_STAMP(7);
    // Results: one kernel behind the pose solve gathers the counts, the PnpResult and every output array into one
    // host-visible buffer, one synchronisation, host copies from there -- instead of eleven device-to-host copies and
    // four rounds of stream synchronisation through vo_batch_get_filtered + vo_batch_get_pose (0.25 of the call's 1.45 ms).
    vo_ctx::PoseBufs &pb = c->pb[c->last];
    const bool mono = c->prm.mono_rotation && c->em_ready;
    FrameGather g;
    g.nA = c->d_nA;
    g.nB = pb.nB;
    g.outB = pb.outB;
    g.xyz = pb.xyz;
    g.idxB = pb.idxB;
    g.idxA = c->d_idxA;
    g.inliers = pb.inliers;
    g.result = pb.results;
    g.em = mono ? pb.em_results : nullptr;
    g.cap = c->cap;
    VO_HIP_TRY(c, pb.done.wait(c->sel->stream)); // (the chain ran on other streams: `done` covers the filter and both pose chains)
    launch_frame_gather(g, c->d_gather, c->sel->stream);
    VO_HIP_TRY(c, hipStreamSynchronize(c->sel->stream));
    VO_HOST_STAMP(8);
    const uint8_t *hb = c->h_gather;
    const FrameGatherLayout L{(size_t)c->cap};
    const int M = peek<int>(hb + L.n_circ), K = peek<int>(hb + L.n_out);
    const PnpResult r = peek<PnpResult>(hb + L.pnp);
    float *outs[4] = {out_l0, out_r0, out_l1, out_r1};
    for (int k = 0; k < 4; k++)
        if (outs[k] && K > 0)
            memcpy(outs[k], hb + L.row(k), (size_t)K * sizeof(float2));
    if (xyz_out && K > 0)
        memcpy(xyz_out, hb + L.xyz(), (size_t)K * 3 * sizeof(float));
    if (keep_idx && K > 0)
        memcpy(keep_idx, hb + L.keep_idx(), (size_t)K * sizeof(int32_t));
    if (keep_idx_circ && M > 0)
        memcpy(keep_idx_circ, hb + L.keep_idx_circ(), (size_t)M * sizeof(int32_t));
    if (n_out)
        *n_out = K;
    if (n_circ)
        *n_circ = M;
    const EmResult e = peek<EmResult>(hb + L.em); // (meaningful under mono only)
    const int em_status = deliver_pose(c, r, mono ? &e : nullptr, rvec_io, tvec_io, R_out, /*pnp_rotation*/ false, /*io_pose*/ true);
    if (inliers && r.n_inliers > 0)
        memcpy(inliers, hb + L.inliers(), (size_t)r.n_inliers * sizeof(int32_t));
    if (n_inliers)
        *n_inliers = r.n_inliers;
    VO_HOST_STAMP(9);
    if (r.status < 0)
        return fail_too_few_pnp(c);
    if (em_status != 1) // mono_rotation and findEssentialMat found nothing: R_out was left untouched
        return VO_NO_ESSENTIAL;
    return r.status == 1 ? VO_OK : VO_NO_MODEL;
}

} // extern "C"
