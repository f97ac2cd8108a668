// capi_corners.hip -- the Shi-Tomasi detector of include/vo_corners.h (vocorn_*): host side of corners.hip.  Its device memory comes
// from the context's Owner at the first vocorn_* call (a context that never makes one allocates and launches what it always did) and
// is regrown when a batch run covers more images than any before it; everything runs on the tracking stream.  The candidate lists
// have the context's corner-list capacity (vo_ctx::fcap), in buffers of their own: the FAST lists (d_feat, d_fages) are float2 + age
// rows that a detect / bucket run of the batch API may still own, and the sort needs 64-bit keys at a power-of-two length.
#include "capi_internal.h"
#include "../../include/vo_corners_response.h"
#include "vo_corners_dev.h"

// The frame loop under VODET_SHI_TOMASI (capi_detector.hip) runs in these buffers too, on the tracking stream or -- the lock-step
// loop's look-ahead -- on the ingest stream, and clears run_n: its results never come out through vocorn_batch_get.
//
// (namespace vo_capi: capi_corners_mask.hip -- vocmask_*, the same detector under a mask -- shares the argument checks, the image
// set-up, the buffers and the fetch, and capi_corners_response.hip -- voresp_*, the detector with blockSize / useHarrisDetector / k --
// the calls themselves; they are declared in capi_internal.h)
namespace vo_capi {

int ensure_corn(vo_ctx *c, int slots)
{
    vo_ctx::Corn &k = c->corn;
    if (k.slots >= slots)
        return VO_OK;
    VO_HIP_TRY(c, hipSetDevice(c->device));
    int rc = sync_all(c); // (a queued run may still use the buffers that are given back)
    if (rc != VO_OK)
        return rc;
    Owner &o = c->own;
    (void)o.give_back(&k.d_ints);
    (void)o.give_back(&k.d_keys);
    (void)o.give_back(&k.d_ckeys);
    (void)o.give_back(&k.d_status);
    (void)o.give_back(&k.d_pts);
    (void)o.give_back(&k.d_maps);
    k.slots = 0;
    k.run_n = 0;
    k.kcap = corn_pow2(c->fcap);
    const size_t S = (size_t)slots;
    bool ok = o.device(&k.d_ints, 3 * S, /*zero*/ true);
    ok = ok && o.device(&k.d_keys, S * k.kcap);
    ok = ok && o.device(&k.d_ckeys, S * k.kcap);
    ok = ok && o.device(&k.d_status, S * c->fcap);
    ok = ok && o.device(&k.d_pts, S * c->fcap);
    ok = ok && o.device(&k.d_maps, S * (size_t)c->max_w * c->max_h);
    if (!ok) // (what was handed out stays with the Owner and goes with the context; the next call tries again)
        return fail_hip(c, "vocorn: device memory for the candidate lists", o.err);
    k.slots = slots;
    return VO_OK;
}

CornArgs corn_args(vo_ctx *c, const vocorn_params &p, const voresp_params *resp)
{
    vo_ctx::Corn &k = c->corn;
    const size_t S = (size_t)k.slots;
    CornArgs a;
    a.max_key = k.d_ints;
    a.ncand = (int *)(k.d_ints + S);
    a.nout = (int *)(k.d_ints + 2 * S);
    a.rounds = nullptr;
    a.maps = k.d_maps;
    a.map_stride = (size_t)c->max_w * c->max_h;
    a.keys = k.d_keys;
    a.ckeys = k.d_ckeys;
    a.status = k.d_status;
    a.pts = k.d_pts;
    a.lcap = c->fcap;
    a.kcap = k.kcap;
    a.quality = p.quality_level;
    a.max_corners = p.max_corners;
    // goodFeaturesToTrack: `if (minDistance >= 1)` the grid loop with cell_size = cvRound(minDistance) and the test
    // dx * dx + dy * dy < minDistance * minDistance (a double); integer offsets: d2 < ceil(minDistance^2)
    a.cell = p.min_distance >= 1 ? (int)lrint(p.min_distance) : 1;
    a.lim = p.min_distance >= 1 ? (int)ceil(p.min_distance * p.min_distance) : 0;
    if (resp) {
        a.block_size = resp->block_size;
        a.use_harris = resp->use_harris;
        a.harris_k = resp->k;
    }
    return a;
}

int corn_check_params(vo_ctx *c, const char *who, const vocorn_params *in, vocorn_params *p)
{
    if (in)
        *p = *in;
    else
        vocorn_default_params(p);
    if (!(p->quality_level > 0) || !(p->min_distance >= 0) || p->max_corners < 0)
        return fail(c, VO_ERR_ARG, (std::string(who) + ": quality_level <= 0, min_distance < 0 or max_corners < 0 (OpenCV's CV_Assert)").c_str());
    if (p->min_distance > VOCORN_MAX_MIN_DISTANCE)
        return fail(c, VO_ERR_ARG, (std::string(who) + ": min_distance beyond VOCORN_MAX_MIN_DISTANCE (256)").c_str());
    return VO_OK;
}

// the image of a synchronous call in the image table: uploaded as it is (never rectified), or the kept pair's left image.
// *image: its index in the table.
int corn_sync_image(vo_ctx *c, const char *who, const uint8_t *img, int w, int h, int stride, int *image)
{
    if (c->seq.on)
        return fail(c, VO_ERR_STATE, (std::string(who) + " inside the sequence loop (vo_seq_*)").c_str());
    int rc = single_image_setup(c, img, w, h, stride, /*plain*/ true);
    if (rc != VO_OK)
        return rc;
    *image = img ? (c->tf_base == 0 ? 2 : 0) : c->tf_base; // (single_image_setup's slot rule)
    return VO_OK;
}

// counts of slot s after a run, then its corners: the two waits of a result that may not fit
int corn_fetch(vo_ctx *c, const char *who, int s, float *pts_out, int cap, int *n_out)
{
    vo_ctx::Corn &k = c->corn;
    const size_t S = (size_t)k.slots;
    int nout = 0;
    VO_HIP_TRY(c, hipMemcpyAsync(&nout, k.d_ints + 2 * S + s, sizeof(int), hipMemcpyDeviceToHost, c->sel->stream));
    VO_HIP_TRY(c, hipStreamSynchronize(c->sel->stream));
    if (nout < 0)
        return fail(c, VO_ERR_OVERFLOW, (std::string(who) + ": more candidates than the context's corner-list capacity "
                                                            "(max(4 x max_pts, 16384, max_w x max_h / 16)): nothing was written").c_str());
    const int m = nout < cap ? nout : cap;
    if (m > 0) {
        VO_HIP_TRY(c, hipMemcpyAsync(pts_out, k.d_pts + (size_t)s * c->fcap, sizeof(float2) * (size_t)m, hipMemcpyDeviceToHost, c->sel->stream));
        VO_HIP_TRY(c, hipStreamSynchronize(c->sel->stream));
    }
    *n_out = nout;
    return VO_OK;
}

int corn_detect(vo_ctx *c, const char *who, const uint8_t *img, int w, int h, int stride, const vocorn_params *params, const voresp_params *resp,
                float *pts_out, int cap, int *n_out)
{
    if (!n_out || cap < 0 || (cap > 0 && !pts_out))
        return fail(c, VO_ERR_ARG, (std::string(who) + ": null output, or cap < 0").c_str());
    vocorn_params p;
    int rc = corn_check_params(c, who, params, &p);
    if (rc != VO_OK)
        return rc;
    int image = 0;
    rc = corn_sync_image(c, who, img, w, h, stride, &image);
    if (rc != VO_OK)
        return rc;
    rc = ensure_corn(c, 1);
    if (rc != VO_OK)
        return rc;
    c->corn.run_n = 0; // (slot 0 no longer holds a batch run's image)
    VO_HIP_TRY(c, launch_corners(c->d_imgs, image, 1, w, h, corn_args(c, p, resp), c->sel->stream));
    return corn_fetch(c, who, 0, pts_out, cap, n_out);
}

int corn_map(vo_ctx *c, const char *who, const uint8_t *img, int w, int h, int stride, const voresp_params *resp, float *out, int out_stride_floats)
{
    if (!out || out_stride_floats < w)
        return fail(c, VO_ERR_ARG, (std::string(who) + ": null output, or a row stride smaller than the width").c_str());
    int image = 0;
    int rc = corn_sync_image(c, who, img, w, h, stride, &image);
    if (rc != VO_OK)
        return rc;
    rc = ensure_corn(c, 1);
    if (rc != VO_OK)
        return rc;
    vo_ctx::Corn &k = c->corn;
    k.run_n = 0; // (slot 0's map no longer belongs to a batch run)
    if (resp)
        launch_corner_map(c->d_imgs, image, w, h, k.d_maps, c->sel->stream, resp->block_size, resp->use_harris, resp->k);
    else
        launch_corner_map(c->d_imgs, image, w, h, k.d_maps, c->sel->stream);
    VO_HIP_TRY(c, hipGetLastError());
    VO_HIP_TRY(c, hipMemcpy2DAsync(out, sizeof(float) * (size_t)out_stride_floats, k.d_maps, sizeof(float) * (size_t)w, sizeof(float) * (size_t)w, (size_t)h,
                                   hipMemcpyDeviceToHost, c->sel->stream));
    VO_HIP_TRY(c, hipStreamSynchronize(c->sel->stream));
    return VO_OK;
}

int corn_batch_run(vo_ctx *c, const char *who, const vocorn_params *params, int first_image, int n_images, bool masked, const voresp_params *resp)
{
    const std::string name(who);
    vocorn_params p;
    int rc = corn_check_params(c, who, params, &p);
    if (rc != VO_OK)
        return rc;
    if (c->seq.on)
        return fail(c, VO_ERR_STATE, (name + " inside the sequence loop (vo_seq_*)").c_str());
    if (c->n_images == 0)
        return fail(c, VO_ERR_STATE, (name + " before vo_batch_configure").c_str());
    if (first_image < 0 || n_images < 1 || first_image > c->n_images - n_images)
        return fail(c, VO_ERR_ARG, (name + ": image range outside the configured table").c_str());
    rc = ensure_corn(c, n_images);
    if (rc != VO_OK)
        return rc;
    VO_HIP_TRY(c, hipSetDevice(c->device));
    vo_ctx::Corn &k = c->corn;
    k.run_n = 0;
    CornArgs a = corn_args(c, p, resp);
    if (masked && c->cmask.any) { // (no image has a mask: the unmasked kernels)
        a.masks = c->cmask.d_table + first_image;
        a.mask_pitch = c->w;
    }
    VO_HIP_TRY(c, launch_corners(c->d_imgs, first_image, n_images, c->w, c->h, a, c->sel->stream));
    k.run_first = first_image;
    k.run_n = n_images;
    k.cfg[0] = c->n_images, k.cfg[1] = c->w, k.cfg[2] = c->h;
    return VO_OK;
}

} // namespace vo_capi

extern "C" {

void vocorn_default_params(vocorn_params *p)
{
    if (!p)
        return;
    p->max_corners = 5000; // feature.cpp:53-55
    p->quality_level = 0.01;
    p->min_distance = 5.0;
}

int vocorn_detect(vo_ctx *c, const uint8_t *img, int w, int h, int stride, const vocorn_params *params, float *pts_out, int cap, int *n_out)
{
    if (!c)
        return VO_ERR_ARG;
    return corn_detect(c, "vocorn_detect", img, w, h, stride, params, nullptr, pts_out, cap, n_out);
}

int vocorn_min_eigen_map(vo_ctx *c, const uint8_t *img, int w, int h, int stride, float *eig_out, int eig_stride_floats)
{
    if (!c)
        return VO_ERR_ARG;
    return corn_map(c, "vocorn_min_eigen_map", img, w, h, stride, nullptr, eig_out, eig_stride_floats);
}

int vocorn_batch_run(vo_ctx *c, const vocorn_params *params, int first_image, int n_images)
{
    if (!c)
        return VO_ERR_ARG;
    return corn_batch_run(c, "vocorn_batch_run", params, first_image, n_images, /*masked*/ false);
}

int vocorn_batch_get(vo_ctx *c, int image_idx, float *pts_out, int cap, int *n_out)
{
    if (!c)
        return VO_ERR_ARG;
    if (!n_out || cap < 0 || (cap > 0 && !pts_out))
        return fail(c, VO_ERR_ARG, "vocorn_batch_get: null output, or cap < 0");
    if (c->seq.on)
        return fail(c, VO_ERR_STATE, "vocorn_batch_get inside the sequence loop (vo_seq_*)");
    const vo_ctx::Corn &k = c->corn;
    if (k.run_n == 0 || k.cfg[0] != c->n_images || k.cfg[1] != c->w || k.cfg[2] != c->h)
        return fail(c, VO_ERR_STATE, "vocorn_batch_get: no vocorn_batch_run on the table as it is configured now");
    if (image_idx < k.run_first || image_idx >= k.run_first + k.run_n)
        return fail(c, VO_ERR_ARG, "vocorn_batch_get: image outside the range of the latest vocorn_batch_run");
    VO_HIP_TRY(c, hipSetDevice(c->device));
    return corn_fetch(c, "vocorn_batch_get", image_idx - k.run_first, pts_out, cap, n_out);
}

} // extern "C"
