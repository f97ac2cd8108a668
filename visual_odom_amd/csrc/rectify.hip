// rectify.hip -- stereo rectification at ingest (vo_params.rectify, include/vo_hip.h; semantics, packed map and raw plane:
// vo_rectify.h).  A context with maps ingests into RAW planes with the kernels it always used (their destination and pitch are
// parameters) and this kernel follows on the same stream: it gathers from the raw plane and writes level 0 of an image-table
// entry at the device pitch -- the bytes the ingest kernels of a context without maps write, at the same place.  Such a context
// never reaches this file.
//
// rectify_kernel: a persistent grid of single-wave workgroups over (image, row, 256-pixel run) items, image and row
// wave-uniform.  A lane makes 4 adjacent destination pixels: ONE 16-byte load of the packed map (the lanes of a wave read 1 KB
// of a map row back to back), per pixel two 2-byte loads -- the taps (iy, ix), (iy, ix + 1) and the pair below, nothing else of
// the source -- and ONE dword store (256 bytes of a destination row per wave).  The row's tail is an overlapping last group
// (w >= 32).  Border: none in the code -- the raw plane's frame of zeros and the clamp of vo_rectify.h make every tap a read
// inside the plane.  Sum: horizontal first by v_dot4_u32_u8 of the two bytes against (32 - a) | a << 8, then the two rows.
// No LDS, no atomics.  A rectified map's taps of neighbouring pixels are neighbouring bytes, so the 2-byte gathers of a wave
// fall into a few cache lines of two source rows; both sides' packed maps (3.7 MB at 1241 x 376) are shared by all images of a
// launch and stay in L2.
// XCD placement: NOT that of pyr_pass_kernel (image z on XCD z % 8).  It would pin each image's source lines to one L2, but a
// source byte is read about once here (twice: the row above re-reads it) and every XCD needs both maps either way; the item
// order below keeps the items of one image adjacent, nothing more.
#include "vo_kernels.h"
#include "vo_rectify.h"

namespace vo {

// the two bytes of a tap pair and the four destination bytes of a lane, at any address
struct __attribute__((packed, aligned(1))) RectB2 {
    uint16_t v;
};
struct __attribute__((packed, aligned(1))) RectB4 {
    uint32_t v;
};

// tab[i]: raw plane (pixel (0, 0)), destination image index, side (0 left, 1 right); maps: the packed map of the left side,
// then of the right side, w * h dwords each, rows tight
__global__ __launch_bounds__(64) void rectify_kernel(const RectImage *__restrict__ tab, int n_items /* images * h * runs */, int n_waves /* = the grid */,
                                                     int w, int h, int raw_pitch, const uint32_t *__restrict__ maps, int pitch,
                                                     uint8_t *__restrict__ pix0 /* pixel (0,0) of image 0 */, size_t img_bytes)
{
    const int runs = (w + 255) / 256, per_img = runs * h;
    for (int it = blockIdx.x; it < n_items; it += n_waves) {
        const int img = it / per_img, rem = it - img * per_img, row = rem / runs, run = rem - row * runs;
        const RectImage e = tab[img];
        int x = run * 256 + (int)threadIdx.x * 4;
        if (x >= w)
            continue;
        x = x < w - 4 ? x : w - 4; // the lane that would cross the row end makes the row's last 4 pixels again
        const VO_GLOBAL uint32_t *__restrict__ mrow = (const VO_GLOBAL uint32_t *)maps + ((size_t)e.side * h + row) * w;
        // four packed map entries: dword-aligned (w need not be a multiple of 4)
        const U32x4A4 m4 = *reinterpret_cast<const VO_GLOBAL U32x4A4 *>(mrow + x);
        const VO_GLOBAL uint8_t *__restrict__ s = (const VO_GLOBAL uint8_t *)e.raw;
        uint32_t out = 0;
        for (int j = 0; j < 4; j++) {
            const uint32_t m = j == 0 ? m4.a : j == 1 ? m4.b : j == 2 ? m4.c : m4.d; // (unrolled: no select is left)
            const RectTap t = rect_tap(m, x + j, row, w, h);
            const VO_GLOBAL uint8_t *__restrict__ p = s + (ptrdiff_t)t.iy * raw_pitch + t.ix;
            const uint32_t r0 = reinterpret_cast<const VO_GLOBAL RectB2 *>(p)->v;
            const uint32_t r1 = reinterpret_cast<const VO_GLOBAL RectB2 *>(p + raw_pitch)->v;
            out |= rect_blend(r0, r1, t.wx, t.b) << (8 * j);
        }
        VO_GLOBAL uint8_t *__restrict__ d = (VO_GLOBAL uint8_t *)pix0 + (size_t)e.image * img_bytes + (size_t)row * pitch + (uint32_t)x;
        reinterpret_cast<VO_GLOBAL RectB4 *>(d)->v = out;
    }
}

#ifndef VO_HOST_EMUL // (the CPU emulator of tests/host_check launches the kernel above itself)
void launch_rectify(const RectImage *tab, int n_images, int w, int h, int raw_pitch, const uint32_t *maps, int pitch, uint8_t *pix0,
                    size_t img_bytes, hipStream_t stream)
{
    if (n_images <= 0)
        return;
    const long long items = (long long)n_images * h * ((w + 255) / 256);
    const int n_items = (int)items, n_waves = n_items < 16384 ? n_items : 16384; // (4096 images of 4096 x 4096 are 2^28 items)
    hipLaunchKernelGGL(rectify_kernel, dim3(n_waves), dim3(64), 0, stream, tab, n_items, n_waves, w, h, raw_pitch, maps, pitch, pix0, img_bytes);
}
#endif // VO_HOST_EMUL

} // namespace vo
