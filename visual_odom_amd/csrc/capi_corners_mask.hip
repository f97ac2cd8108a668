// capi_corners_mask.hip -- the Shi-Tomasi detector under cv::goodFeaturesToTrack's mask argument (include/vo_corners_mask.h,
// vocmask_*): host side of the masked kernels of corners.hip.  Argument checks, image set-up, candidate buffers and the fetch are
// capi_corners.hip's (capi_internal.h).  The masks live in a device table of one max_w x max_h plane per image of the image table,
// rows tight, which comes from the context's Owner at the first vocmask_* call (a context that never makes one allocates and launches
// what it always did); a run reads the plane of image i through d_table[i], null for an image without a mask.  The synchronous calls
// use a plane, a point list and a table entry of their own behind those of the images.  Everything runs on the tracking stream.
#include "capi_internal.h"
#include "../../include/vo_corners_response.h"
#include "vo_corners_dev.h"

namespace {

size_t plane_bytes(const vo_ctx *c) { return (size_t)c->max_w * c->max_h; }

int ensure_cmask(vo_ctx *c)
{
    vo_ctx::CornMask &m = c->cmask;
    if (m.ready)
        return VO_OK;
    VO_HIP_TRY(c, hipSetDevice(c->device));
    Owner &o = c->own;
    const size_t S = (size_t)c->max_images + 1;
    bool ok = (m.d_masks || o.device(&m.d_masks, S * plane_bytes(c)));
    ok = ok && (m.d_kept || o.device(&m.d_kept, S * (size_t)(c->cap > 0 ? c->cap : 1)));
    ok = ok && (m.d_table || o.device(&m.d_table, S, /*zero*/ true));
    if (!ok) // (what was handed out stays with the Owner and goes with the context; the next call asks for the rest)
        return fail_hip(c, "vocmask: device memory for the masks", o.err);
    const uint8_t *own_plane = m.d_masks + (size_t)c->max_images * plane_bytes(c);
    VO_HIP_TRY(c, hipMemcpy(m.d_table + c->max_images, &own_plane, sizeof(own_plane), hipMemcpyHostToDevice));
    m.has.assign((size_t)c->max_images, (uint8_t)0);
    m.any = false;
    m.ready = true;
    return VO_OK;
}

int check_kept(vo_ctx *c, const char *who, const float *kept_xy, int n_kept, int radius)
{
    if (n_kept < 0 || n_kept > c->cap || (n_kept > 0 && !kept_xy))
        return fail(c, VO_ERR_ARG, (std::string(who) + ": n_kept outside 0 .. max_pts, or null points").c_str());
    if (radius < 0 || radius > VOCORN_MAX_MIN_DISTANCE)
        return fail(c, VO_ERR_ARG, (std::string(who) + ": radius outside 0 .. VOCORN_MAX_MIN_DISTANCE (256)").c_str());
    return VO_OK;
}

// the kept points into row `row` of d_kept (the caller's memory is free again on return), then the disc mask of plane `row` for a
// w x h image, enqueued
int build_disc_mask(vo_ctx *c, int row, const float *kept_xy, int n_kept, int radius, int w, int h)
{
    vo_ctx::CornMask &m = c->cmask;
    float2 *d_kept = m.d_kept + (size_t)row * (c->cap > 0 ? c->cap : 1);
    if (n_kept > 0) {
        VO_HIP_TRY(c, hipMemcpyAsync(d_kept, kept_xy, sizeof(float2) * (size_t)n_kept, hipMemcpyHostToDevice, c->sel->stream));
        VO_HIP_TRY(c, hipStreamSynchronize(c->sel->stream)); // (pageable host memory: safe to return from)
    }
    VO_HIP_TRY(c, launch_corner_disc_mask(d_kept, n_kept, radius, m.d_masks + (size_t)row * plane_bytes(c), w, h, c->sel->stream));
    return VO_OK;
}

// marks image idx as masked (or not) on the host and in the table the runs read
int set_entry(vo_ctx *c, int idx, bool on)
{
    vo_ctx::CornMask &m = c->cmask;
    if ((m.has[(size_t)idx] != 0) == on)
        return VO_OK;
    const uint8_t *p = on ? m.d_masks + (size_t)idx * plane_bytes(c) : nullptr;
    VO_HIP_TRY(c, hipMemcpyAsync(m.d_table + idx, &p, sizeof(p), hipMemcpyHostToDevice, c->sel->stream));
    VO_HIP_TRY(c, hipStreamSynchronize(c->sel->stream)); // (p is a local)
    m.has[(size_t)idx] = on ? 1 : 0;
    m.any = false;
    for (uint8_t v : m.has)
        m.any = m.any || v;
    return VO_OK;
}

int batch_checks(vo_ctx *c, const char *who, int image_idx)
{
    if (c->seq.on)
        return fail(c, VO_ERR_STATE, (std::string(who) + " inside the sequence loop (vo_seq_*)").c_str());
    if (c->n_images == 0)
        return fail(c, VO_ERR_STATE, (std::string(who) + " before vo_batch_configure").c_str());
    if (image_idx < 0 || image_idx >= c->n_images)
        return fail(c, VO_ERR_ARG, (std::string(who) + ": image outside the configured table").c_str());
    return VO_OK;
}

// the detector on image `image` of the table under the synchronous calls' own plane, and its results
int detect_under_own_mask(vo_ctx *c, const char *who, int image, int w, int h, const vocorn_params &p, const voresp_params *resp, float *pts_out, int cap,
                          int *n_out)
{
    int rc = ensure_corn(c, 1);
    if (rc != VO_OK)
        return rc;
    c->corn.run_n = 0; // (slot 0 no longer holds a batch run's image)
    CornArgs a = corn_args(c, p, resp);
    a.masks = c->cmask.d_table + c->max_images;
    a.mask_pitch = w;
    VO_HIP_TRY(c, launch_corners(c->d_imgs, image, 1, w, h, a, c->sel->stream));
    return corn_fetch(c, who, 0, pts_out, cap, n_out);
}

} // namespace

int vo_capi::cmask_detect(vo_ctx *c, const char *who, const uint8_t *img, int w, int h, int stride, const uint8_t *mask, int mask_stride,
                          const vocorn_params *params, const voresp_params *resp, float *pts_out, int cap, int *n_out)
{
    if (!mask)
        return corn_detect(c, who, img, w, h, stride, params, resp, pts_out, cap, n_out);
    if (!n_out || cap < 0 || (cap > 0 && !pts_out))
        return fail(c, VO_ERR_ARG, (std::string(who) + ": null output, or cap < 0").c_str());
    if (mask_stride < w)
        return fail(c, VO_ERR_ARG, (std::string(who) + ": mask stride smaller than the width").c_str());
    vocorn_params p;
    int rc = corn_check_params(c, who, params, &p);
    if (rc != VO_OK)
        return rc;
    int image = 0;
    rc = corn_sync_image(c, who, img, w, h, stride, &image);
    if (rc != VO_OK)
        return rc;
    rc = ensure_cmask(c);
    if (rc != VO_OK)
        return rc;
    uint8_t *plane = c->cmask.d_masks + (size_t)c->max_images * plane_bytes(c);
    VO_HIP_TRY(c, hipMemcpy2DAsync(plane, (size_t)w, mask, (size_t)mask_stride, (size_t)w, (size_t)h, hipMemcpyHostToDevice, c->sel->stream));
    return detect_under_own_mask(c, who, image, w, h, p, resp, pts_out, cap, n_out); // (its fetch waits for the stream)
}

extern "C" {

int vocmask_detect(vo_ctx *c, const uint8_t *img, int w, int h, int stride, const uint8_t *mask, int mask_stride, const vocorn_params *params,
                   float *pts_out, int cap, int *n_out)
{
    if (!c)
        return VO_ERR_ARG;
    if (!mask) // (vocorn_detect itself)
        return corn_detect(c, "vocorn_detect", img, w, h, stride, params, nullptr, pts_out, cap, n_out);
    return cmask_detect(c, "vocmask_detect", img, w, h, stride, mask, mask_stride, params, nullptr, pts_out, cap, n_out);
}

int vocmask_disc_mask(vo_ctx *c, int w, int h, const float *kept_xy, int n_kept, int radius, uint8_t *mask_out, int mask_stride)
{
    if (!c)
        return VO_ERR_ARG;
    if (!mask_out || mask_stride < w)
        return fail(c, VO_ERR_ARG, "vocmask_disc_mask: null output, or a mask stride smaller than the width");
    int rc = check_kept(c, "vocmask_disc_mask", kept_xy, n_kept, radius);
    if (rc != VO_OK)
        return rc;
    if (c->seq.on)
        return fail(c, VO_ERR_STATE, "vocmask_disc_mask inside the sequence loop (vo_seq_*)");
    rc = vo_batch_configure(c, 4, w, h, 1); // (the size checks, and the image table as the other synchronous calls leave it)
    if (rc != VO_OK)
        return rc;
    rc = ensure_cmask(c);
    if (rc != VO_OK)
        return rc;
    rc = build_disc_mask(c, c->max_images, kept_xy, n_kept, radius, w, h);
    if (rc != VO_OK)
        return rc;
    const uint8_t *plane = c->cmask.d_masks + (size_t)c->max_images * plane_bytes(c);
    VO_HIP_TRY(c, hipMemcpy2DAsync(mask_out, (size_t)mask_stride, plane, (size_t)w, (size_t)w, (size_t)h, hipMemcpyDeviceToHost, c->sel->stream));
    VO_HIP_TRY(c, hipStreamSynchronize(c->sel->stream));
    return VO_OK;
}

int vocmask_replenish(vo_ctx *c, const uint8_t *img, int w, int h, int stride, const float *kept_xy, int n_kept, int radius,
                      const vocorn_params *params, float *pts_out, int cap, int *n_out)
{
    if (!c)
        return VO_ERR_ARG;
    if (!n_out || cap < 0 || (cap > 0 && !pts_out))
        return fail(c, VO_ERR_ARG, "vocmask_replenish: null output, or cap < 0");
    int rc = check_kept(c, "vocmask_replenish", kept_xy, n_kept, radius);
    if (rc != VO_OK)
        return rc;
    vocorn_params p;
    rc = corn_check_params(c, "vocmask_replenish", params, &p);
    if (rc != VO_OK)
        return rc;
    int image = 0;
    rc = corn_sync_image(c, "vocmask_replenish", img, w, h, stride, &image);
    if (rc != VO_OK)
        return rc;
    rc = ensure_cmask(c);
    if (rc != VO_OK)
        return rc;
    rc = build_disc_mask(c, c->max_images, kept_xy, n_kept, radius, w, h);
    if (rc != VO_OK)
        return rc;
    return detect_under_own_mask(c, "vocmask_replenish", image, w, h, p, nullptr, pts_out, cap, n_out);
}

int vocmask_batch_set_mask(vo_ctx *c, int image_idx, const uint8_t *mask, int mask_stride)
{
    if (!c)
        return VO_ERR_ARG;
    int rc = batch_checks(c, "vocmask_batch_set_mask", image_idx);
    if (rc != VO_OK)
        return rc;
    if (mask && mask_stride < c->w)
        return fail(c, VO_ERR_ARG, "vocmask_batch_set_mask: mask stride smaller than the width");
    if (!mask && !c->cmask.ready) // (nothing to remove)
        return VO_OK;
    rc = ensure_cmask(c);
    if (rc != VO_OK)
        return rc;
    VO_HIP_TRY(c, hipSetDevice(c->device));
    if (mask) {
        uint8_t *plane = c->cmask.d_masks + (size_t)image_idx * plane_bytes(c);
        VO_HIP_TRY(c, hipMemcpy2DAsync(plane, (size_t)c->w, mask, (size_t)mask_stride, (size_t)c->w, (size_t)c->h, hipMemcpyHostToDevice, c->sel->stream));
        VO_HIP_TRY(c, hipStreamSynchronize(c->sel->stream)); // (pageable host memory: safe to return from)
    }
    return set_entry(c, image_idx, mask != nullptr);
}

int vocmask_batch_set_kept(vo_ctx *c, int image_idx, const float *kept_xy, int n_kept, int radius)
{
    if (!c)
        return VO_ERR_ARG;
    int rc = check_kept(c, "vocmask_batch_set_kept", kept_xy, n_kept, radius);
    if (rc != VO_OK)
        return rc;
    rc = batch_checks(c, "vocmask_batch_set_kept", image_idx);
    if (rc != VO_OK)
        return rc;
    rc = ensure_cmask(c);
    if (rc != VO_OK)
        return rc;
    VO_HIP_TRY(c, hipSetDevice(c->device));
    rc = build_disc_mask(c, image_idx, kept_xy, n_kept, radius, c->w, c->h);
    if (rc != VO_OK)
        return rc;
    return set_entry(c, image_idx, true);
}

int vocmask_batch_run(vo_ctx *c, const vocorn_params *params, int first_image, int n_images)
{
    if (!c)
        return VO_ERR_ARG;
    return corn_batch_run(c, "vocmask_batch_run", params, first_image, n_images, /*masked*/ true);
}

} // extern "C"
