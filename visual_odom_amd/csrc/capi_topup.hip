// capi_topup.hip -- the frame loop's top-up under a mask of the carried points (include/vo_topup.h, votop_*): the checked record in
// vo_ctx, the mask planes of the frames with the table the kernels read them through, and votop_get_mask.  What the record makes the
// three call sites of the loop launch is det_launch's masked route (capi_detector.hip).
#include "capi_internal.h"

namespace vo_capi {

// One plane of max_w x max_h bytes per frame, 16 bytes apart at least, and d_table[f] = plane f.  Growing drains the context (a queued
// run may still read the planes that are given back): never inside a lock-step step.
int top_ensure(vo_ctx *c, int frames)
{
    vo_ctx::TopUp &t = c->top;
    if (t.slots >= frames)
        return VO_OK;
    VO_HIP_TRY(c, hipSetDevice(c->device));
    int rc = sync_all(c);
    if (rc != VO_OK)
        return rc;
    Owner &o = c->own;
    (void)o.give_back(&t.d_planes);
    (void)o.give_back(&t.d_table);
    t.slots = 0;
    t.ran = 0;
    t.plane_stride = ((size_t)c->max_w * c->max_h + 15) & ~(size_t)15;
    if (!o.device(&t.d_planes, (size_t)frames * t.plane_stride) || !o.device(&t.d_table, (size_t)frames))
        return fail_hip(c, "votop: device memory for the mask planes", o.err);
    std::vector<const uint8_t *> tab((size_t)frames);
    for (int f = 0; f < frames; f++)
        tab[(size_t)f] = t.d_planes + (size_t)f * t.plane_stride;
    VO_HIP_TRY(c, hipMemcpy(t.d_table, tab.data(), sizeof(tab[0]) * tab.size(), hipMemcpyHostToDevice));
    t.slots = frames;
    return VO_OK;
}

} // namespace vo_capi

extern "C" {

void votop_default_params(votop_params *p)
{
    if (!p)
        return;
    p->mode = VOTOP_OFF;
    p->radius = 5;
}

int votop_set_params(vo_ctx *c, const votop_params *p)
{
    if (!c)
        return VO_ERR_ARG;
    votop_params d;
    if (p)
        d = *p;
    else
        votop_default_params(&d);
    if (d.mode != VOTOP_OFF && d.mode != VOTOP_CARRIED)
        return fail(c, VO_ERR_ARG, "votop_set_params: unknown mode (VOTOP_OFF, VOTOP_CARRIED)");
    if (d.radius < 0 || d.radius > VOCORN_MAX_MIN_DISTANCE)
        return fail(c, VO_ERR_ARG, "votop_set_params: radius outside 0 .. VOCORN_MAX_MIN_DISTANCE (256)");
    if (c->seq.on)
        return fail(c, VO_ERR_STATE, "votop_set_params inside the sequence loop (vo_seq_*): the loop took its mask planes and probed its "
                                     "schedule with the record in force");
    c->top.prm = d;
    c->top.ran = 0;
    return VO_OK;
}

int votop_get_params(const vo_ctx *c, votop_params *p)
{
    if (!c || !p)
        return VO_ERR_ARG;
    *p = c->top.prm;
    return VO_OK;
}

int votop_get_mask(vo_ctx *c, int frame, uint8_t *mask_out, int mask_stride)
{
    if (!c)
        return VO_ERR_ARG;
    if (!mask_out || mask_stride < c->w)
        return fail(c, VO_ERR_ARG, "votop_get_mask: null output, or a mask stride smaller than the width");
    if (c->seq.on)
        return fail(c, VO_ERR_STATE, "votop_get_mask inside the sequence loop (vo_seq_*)");
    const vo_ctx::TopUp &t = c->top;
    if (t.ran == 0 || t.cfg[0] != c->n_images || t.cfg[1] != c->w || t.cfg[2] != c->h)
        return fail(c, VO_ERR_STATE, "votop_get_mask: no masked detection on the table as it is configured now");
    if (frame < 0 || frame >= t.ran)
        return fail(c, VO_ERR_ARG, "votop_get_mask: frame outside the latest masked detection");
    if (!c->h_detect[(size_t)frame])
        return fail(c, VO_ERR_STATE, "votop_get_mask: this frame did not detect again");
    VO_HIP_TRY(c, hipSetDevice(c->device));
    VO_HIP_TRY(c, hipMemcpy2DAsync(mask_out, (size_t)mask_stride, t.d_planes + (size_t)frame * t.plane_stride, (size_t)c->w, (size_t)c->w, (size_t)c->h,
                                   hipMemcpyDeviceToHost, c->sel->stream));
    VO_HIP_TRY(c, hipStreamSynchronize(c->sel->stream));
    return VO_OK;
}

} // extern "C"
