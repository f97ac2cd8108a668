// dev/fast_dev.hip -- fast.hip plus the 128 x 32 tile of the FAST kernel: measured slower than both product tiles (fast.hip,
// launch_fast_corners).
//
// The developer build (python -m visual_odom_amd.build --dev -> libvo_hip_dev.so) compiles this file INSTEAD of fast.hip and the
// CPU emulator of tests/host_check gets the kernel below through the last lines of fast.hip; the product library never sees it.  fast.hip is included as it is, with the two
// launchers on the way to the tile kernel under other names: launch_fast_corners below reads VO_FAST_TILE and falls through to
// the product's, so the switch needs no hook in the product source.
#include "../vo_kernels.h"
#include "../vo_dev_hooks.h"
#ifndef VO_HOST_EMUL // (the emulator arrives here from the end of fast.hip)
#define launch_fast_corners launch_fast_corners_product
#define launch_detect_bucket launch_detect_bucket_product
#include "../fast.hip"
#undef launch_fast_corners
#undef launch_detect_bucket
#endif

namespace vo {

__global__ __launch_bounds__(256) void fast_tile_big_kernel(const PyrImage *__restrict__ imgs,
                                                            const Quad *__restrict__ quads,
                                                            const int *__restrict__ detect, int threshold, int nonmax,
                                                            unsigned long long *__restrict__ mask, int segs,
                                                            int *__restrict__ rowcnt)
{
    fast_tile_body<2, 32>(imgs, quads, detect, threshold, nonmax, mask, segs, rowcnt);
}

#ifndef VO_HOST_EMUL
// VO_FAST_TILE = 0 / 1 / 2 forces a tile form (2: the 128 x 32 tile); unset: the product's choice
void launch_fast_corners(const PyrImage *d_imgs, const Quad *d_quads, const int *d_detect, int n_frames, int w, int h,
                         int threshold, int nonmax, unsigned long long *d_nmsmask, int *d_rowcnt, int *d_rowoff,
                         const int *d_ntracked, int *d_nnew, int cap, float2 *d_out, hipStream_t stream)
{
    const int tile = dev_knob("VO_FAST_TILE", -1);
    if (tile < 0) {
        launch_fast_corners_product(d_imgs, d_quads, d_detect, n_frames, w, h, threshold, nonmax, d_nmsmask, d_rowcnt, d_rowoff,
                                    d_ntracked, d_nnew, cap, d_out, stream);
        return;
    }
    if (n_frames <= 0)
        return;
    const int segs = (w + 63) / 64;
    if (tile == 2)
        hipLaunchKernelGGL(fast_tile_big_kernel, dim3((segs + 1) / 2, (h + 31) / 32, n_frames), dim3(256), 0, stream, d_imgs,
                           d_quads, d_detect, threshold, nonmax, d_nmsmask, segs, d_rowcnt);
    else
    if (tile == 1)
        hipLaunchKernelGGL(fast_tile_tall_kernel, dim3(segs, (h + 31) / 32, n_frames), dim3(256), 0, stream, d_imgs,
                           d_quads, d_detect, threshold, nonmax, d_nmsmask, segs, d_rowcnt);
    else
        hipLaunchKernelGGL(fast_tile_kernel, dim3(segs, (h + 15) / 16, n_frames), dim3(256), 0, stream, d_imgs,
                           d_quads, d_detect, threshold, nonmax, d_nmsmask, segs, d_rowcnt);
    hipLaunchKernelGGL(fast_rowscan_kernel, dim3(n_frames), dim3(256), 0, stream, d_rowcnt, d_rowoff, h, d_detect,
                       d_nnew);
    const int rows_per_wg = 4 * fast_nms_rows_per_wave(segs);
    hipLaunchKernelGGL(fast_nms_write_kernel, dim3((h + rows_per_wg - 1) / rows_per_wg, n_frames), dim3(256), 0, stream, d_nmsmask, segs, h, d_detect,
                       d_rowoff, d_ntracked, cap, d_out);
}

// (launch_detect_bucket of fast.hip over the launcher above)
void launch_detect_bucket(const PyrImage *d_imgs, const Quad *d_quads, const int *d_detect, int n_frames, int w,
                          int h, int threshold, int nonmax, unsigned long long *d_nmsmask,
                          int *d_rowcnt, int *d_rowoff,
                          const int *d_ntracked, int *d_nnew, int cap, float2 *d_feat, const int *d_ages,
                          int bucket_size, int fpb, float2 *d_out_pts, int *d_out_ages, int *d_out_n, int out_cap,
                          const int *d_active, int *d_overflow, hipStream_t stream)
{
    launch_fast_corners(d_imgs, d_quads, d_detect, n_frames, w, h, threshold, nonmax, d_nmsmask, d_rowcnt, d_rowoff,
                        d_ntracked, d_nnew, cap, d_feat, stream);
    if (bucket_size > 0)
        launch_bucket(d_feat, nullptr, d_ages, d_ntracked, d_nnew, cap, w, h, bucket_size, fpb, d_out_pts, d_out_ages,
                      d_out_n, out_cap, d_active, d_overflow, n_frames, stream);
}
#endif // VO_HOST_EMUL

} // namespace vo
