// capi_detector.hip -- the frame loop's detector (include/vo_detector.h, vodet_*): the checked record in vo_ctx, and what the three
// call sites of the loop -- run_stages' DETECT part (capi_run.hip), the look-ahead of the lock-step loop (capi_sched.hip) and its
// inline detection -- launch under VODET_SHI_TOMASI: the frames form of corners.hip's three passes, in the buffers of the vocorn_*
// calls (capi_corners.hip), with the corners and their count written where bucket_kernel's split form reads them.  With the top-up
// of include/vo_topup.h on, the same call sites get the masked route: map, discs, masked maximum, candidates, select.
#include "capi_internal.h"
#include "vo_corners_dev.h"

namespace vo_capi {

// candidate buffers for `frames` frames -- and, with the top-up on (include/vo_topup.h), their mask planes.  Growing them drains the
// context (ensure_corn, top_ensure): the lock-step loop calls this from vo_seq_configure, the batch stage when a run covers more
// frames than any before it.
int det_ensure(vo_ctx *c, int frames)
{
    int rc = ensure_corn(c, frames);
    if (rc == VO_OK && topup_on(c))
        rc = top_ensure(c, frames);
    return rc;
}

// ahead_maps (top-up only): the maps the look-ahead left for these frames (det_lookahead_maps); null: the map pass runs here
int det_launch(vo_ctx *c, const Quad *quads, const int *d_detect, int frames, float2 *corners, int *n_out, hipStream_t stream, const float *ahead_maps)
{
    if (c->corn.slots < frames)
        return fail(c, VO_ERR_STATE, "the Shi-Tomasi detector's candidate buffers are smaller than the run");
    c->corn.run_n = 0; // the slots no longer hold a vocorn_batch_run: vocorn_batch_get answers VO_ERR_STATE
    CornArgs a = corn_args(c, c->det.corners, &c->det.response);
    a.pts = corners;
    a.nout = n_out;
    if (!topup_on(c)) {
        VO_HIP_TRY(c, launch_corners_frames(c->d_imgs, quads, d_detect, frames, c->w, c->h, a, stream));
        return VO_OK;
    }
    // map, discs of the carried points, the maximum under them, candidates under them, select: one route for every form of the loop
    vo_ctx::TopUp &t = c->top;
    if (t.slots < frames)
        return fail(c, VO_ERR_STATE, "the top-up's mask planes are fewer than the run's frames");
    if (ahead_maps)
        a.maps = const_cast<float *>(ahead_maps);
    else
        VO_HIP_TRY(c, launch_corners_frames_map(c->d_imgs, quads, d_detect, frames, c->w, a, stream));
    a.masks = t.d_table;
    a.mask_pitch = c->w;
    CornTopArgs ta;
    ta.feat = c->d_feat;
    ta.fcap = c->fcap;
    ta.n_tracked = c->d_ntracked;
    ta.radius = t.prm.radius;
    ta.planes = const_cast<uint8_t *const *>(t.d_table);
    ta.plane0 = t.d_planes;
    ta.plane_stride = t.plane_stride;
    ta.max_kept = c->dprm.redetect_below - 1;
    VO_HIP_TRY(c, launch_corners_frames_masked(d_detect, frames, c->w, c->h, a, ta, stream));
    t.ran = c->seq.on ? 0 : frames;
    t.cfg[0] = c->n_images, t.cfg[1] = c->w, t.cfg[2] = c->h;
    return VO_OK;
}

int det_lookahead_maps(vo_ctx *c, const Quad *quads, int frames, float *maps, hipStream_t stream)
{
    CornArgs a = corn_args(c, c->det.corners, &c->det.response);
    a.maps = maps;
    VO_HIP_TRY(c, launch_corners_frames_map(c->d_imgs, quads, nullptr, frames, c->w, a, stream));
    return VO_OK;
}

} // namespace vo_capi

extern "C" {

void vodet_default_params(vodet_params *p)
{
    if (!p)
        return;
    p->detector = VODET_FAST;
    vocorn_default_params(&p->corners);
    voresp_default_params(&p->response);
}

int vodet_set_params(vo_ctx *c, const vodet_params *p)
{
    if (!c)
        return VO_ERR_ARG;
    vodet_params d;
    if (p)
        d = *p;
    else
        vodet_default_params(&d);
    if (d.detector != VODET_FAST && d.detector != VODET_SHI_TOMASI)
        return fail(c, VO_ERR_ARG, "vodet_set_params: unknown detector (VODET_FAST, VODET_SHI_TOMASI)");
    int rc = corn_check_params(c, "vodet_set_params", &d.corners, &d.corners);
    if (rc == VO_OK)
        rc = corn_check_resp(c, "vodet_set_params", &d.response, &d.response);
    if (rc != VO_OK)
        return rc;
    if (c->seq.on)
        return fail(c, VO_ERR_STATE, "vodet_set_params inside the sequence loop (vo_seq_*): look-ahead corners of the other detector may be "
                                     "in flight, and the schedule was probed with it");
    c->det = d;
    return VO_OK;
}

int vodet_get_params(const vo_ctx *c, vodet_params *p)
{
    if (!c || !p)
        return VO_ERR_ARG;
    *p = c->det;
    return VO_OK;
}

} // extern "C"
