// capi_corners_response.hip -- the Shi-Tomasi detector with cv::goodFeaturesToTrack's blockSize, useHarrisDetector and k
// (include/vo_corners_response.h, voresp_*): host side of corn_map_resp_kernel of corners.hip.  Argument checks, image set-up,
// buffers, masks and the fetch are capi_corners.hip's and capi_corners_mask.hip's (capi_internal.h): every call here checks its
// response record and then IS the vocorn_* / vocmask_* call, which takes the record as one more argument.  It allocates nothing of
// its own.
#include "capi_internal.h"
#include "../../include/vo_corners_response.h"

#include <math.h>

namespace vo_capi {

// *r: the record to run with.  The defaults are the run the other two headers make.
int corn_check_resp(vo_ctx *c, const char *who, const voresp_params *in, voresp_params *r)
{
    if (in)
        *r = *in;
    else
        voresp_default_params(r);
    if ((r->block_size != 3 && r->block_size != 5) || (r->use_harris != 0 && r->use_harris != 1) || !isfinite(r->k))
        return fail(c, VO_ERR_ARG, (std::string(who) + ": built are block_size 3 and 5 (the sizes whose row sum OpenCV adds left to right), "
                                                       "use_harris 0 and 1, and a finite k").c_str());
    return VO_OK;
}

} // namespace vo_capi

extern "C" {

void voresp_default_params(voresp_params *p)
{
    if (!p)
        return;
    p->block_size = 3; // cv::goodFeaturesToTrack's defaults
    p->use_harris = 0;
    p->k = 0.04;
}

int voresp_map(vo_ctx *c, const uint8_t *img, int w, int h, int stride, const voresp_params *resp, float *out, int out_stride_floats)
{
    if (!c)
        return VO_ERR_ARG;
    voresp_params r;
    int rc = corn_check_resp(c, "voresp_map", resp, &r);
    if (rc != VO_OK)
        return rc;
    return corn_map(c, "voresp_map", img, w, h, stride, &r, out, out_stride_floats);
}

int voresp_detect(vo_ctx *c, const uint8_t *img, int w, int h, int stride, const uint8_t *mask, int mask_stride, const vocorn_params *params,
                  const voresp_params *resp, float *pts_out, int cap, int *n_out)
{
    if (!c)
        return VO_ERR_ARG;
    voresp_params r;
    int rc = corn_check_resp(c, "voresp_detect", resp, &r);
    if (rc != VO_OK)
        return rc;
    return cmask_detect(c, "voresp_detect", img, w, h, stride, mask, mask_stride, params, &r, pts_out, cap, n_out);
}

int voresp_batch_run(vo_ctx *c, const vocorn_params *params, const voresp_params *resp, int first_image, int n_images)
{
    if (!c)
        return VO_ERR_ARG;
    voresp_params r;
    int rc = corn_check_resp(c, "voresp_batch_run", resp, &r);
    if (rc != VO_OK)
        return rc;
    return corn_batch_run(c, "voresp_batch_run", params, first_image, n_images, /*masked*/ true, &r);
}

} // extern "C"
