// ingest_fmt.hip -- input formats other than 8-bit gray (vo_params.input_format, include/vo_hip.h): the conversion to the
// gray level-0 image happens in the kernel that moves the image anyway; the host only ever copies raw bytes.
//
// The reference's ./run has two input modes and neither hands over a gray plane: files are imread(IMREAD_COLOR) +
// cvtColor(BGR2GRAY) per frame (main.cpp:107-114,135-141 -> utils.cpp:172-190), the sensor mode delivers ONE buffer of
// 16-bit words per frame, left pixel = low byte, right pixel = high byte, de-interleaved on the host pixel by pixel
// (rgbd_standalone.cpp:178-196).
//
//   VO_FMT_GRAY8_X2       pixel x at byte 2 x of the pointer given (one plane of the two-byte interleave)
//   VO_FMT_BGR8 / RGB8    3 bytes per pixel, Y = (B * 1868 + G * 9617 + R * 4899 + 8192) >> 14  (cvtColor's 14-bit integer form)
//   VO_FMT_BGRA8 / RGBA8  4 bytes per pixel, alpha ignored
//
// Two kernels, twins of the gray ones (which are untouched -- a VO_FMT_GRAY8 context never reaches this file):
//   seq_ingest_fmt_kernel   lock-step loop, like seq_ingest_kernel (seq.hip): a persistent grid of single-wave workgroups
//                           that walk over the rows, 192 of them when a pair crosses PCIe, 8192 for resident sources
//   pull_image_fmt_kernel   synchronous calls and the batch upload, like pull_image_kernel (pyramid.hip): one wave per 512
//                           pixels of a row, raw rows in (page-locked staging slot or device memory), gray rows at the device pitch out
// Both go through ONE row converter, ingest_row8<FMT>: 8 destination pixels per lane from 8 * bpp source bytes by unaligned
// vector loads, the row's tail by an overlapping last group.
//
// WHAT IS READ: a source row only inside [row, row + w * bpp) -- the last row of a caller's page-locked buffer may end on a
// page boundary.  For VO_FMT_GRAY8_X2 even less, [row, row + 2 w - 1): the right plane of an interleaved frame is `buf + 1`,
// and byte 2 w of its last row would be one past the frame.  So a single X2 plane takes two overlapping 8-byte loads (bytes
// 0 .. 7 and 7 .. 14 of the group) instead of one of 16.
// Y8I PAIRS ARE READ ONCE: a pair with right == left + 1 is one buffer; the trip of its left row loads the eight 16-bit words
// once (16 bytes, inside the row) and v_perm_b32 byte selects split them into the two 8-byte stores; the trips of its right
// rows do nothing.  Reading the buffer once per plane would double the bytes on the link.
// Colour: the pixel's dword comes out of the loaded dwords by v_alignbyte_b32 (3-byte formats; 4-byte formats have it already),
// the three products by two v_dot4_u32_u8 against the weights split into byte halves (1868 = 7 * 256 + 76, 9617 = 37 * 256 +
// 145, 4899 = 19 * 256 + 35; the fourth weight is 0, which is how alpha -- or the neighbour's first byte -- is ignored), i.e.
// dot4(p, lo) + 8192 + (dot4(p, hi) << 8), exact in 32 bits (<= 255 * 16384 + 8192).
#include "vo_isa.h"
#include "vo_kernels.h"

#include <type_traits>

namespace vo {

// the kernels' names for the formats: the values of the public header
enum { ING_GRAY8 = VO_FMT_GRAY8, ING_GRAY8_X2 = VO_FMT_GRAY8_X2, ING_BGR8 = VO_FMT_BGR8, ING_RGB8 = VO_FMT_RGB8, ING_BGRA8 = VO_FMT_BGRA8,
       ING_RGBA8 = VO_FMT_RGBA8 };

// gray of one pixel whose bytes 0 .. 2 are (B, G, R) -- or (R, G, B) with SWAP -- and whose byte 3 is ignored
template <bool SWAP>
__device__ __forceinline__ uint32_t ing_gray(uint32_t p)
{
    constexpr uint32_t c0 = SWAP ? 4899u : 1868u, c2 = SWAP ? 1868u : 4899u;
    constexpr uint32_t lo = (c0 & 255u) | ((9617u & 255u) << 8) | ((c2 & 255u) << 16);
    constexpr uint32_t hi = (c0 >> 8) | ((9617u >> 8) << 8) | ((c2 >> 8) << 16);
    return (udot4(p, lo, 8192u) + (udot4(p, hi, 0u) << 8)) >> 14;
}
__device__ __forceinline__ uint32_t ing_pack4(uint32_t y0, uint32_t y1, uint32_t y2, uint32_t y3)
{
    return y0 | (y1 << 8) | (y2 << 16) | (y3 << 24);
}

// 8 destination pixels from the source bytes of pixel x .. x + 7 of a row: s = row + x * bpp.  Reads [s, s + 8 * bpp), for
// ING_GRAY8_X2 [s, s + 15).
template <int FMT>
__device__ __forceinline__ U32x2A1 ingest_row8(const VO_GLOBAL uint8_t *__restrict__ s)
{
    U32x2A1 o;
    if constexpr (FMT == ING_GRAY8_X2) {
        const U32x2A1 u = *reinterpret_cast<const VO_GLOBAL U32x2A1 *>(s);     // bytes 0 .. 7: pixels 0 .. 3 at 0, 2, 4, 6
        const U32x2A1 v = *reinterpret_cast<const VO_GLOBAL U32x2A1 *>(s + 7); // bytes 7 .. 14: pixels 4 .. 7 at 1, 3, 5, 7
        o.a = perm_b32(u.b, u.a, 0x06040200u);
        o.b = perm_b32(v.b, v.a, 0x07050301u);
    } else if constexpr (FMT == ING_BGR8 || FMT == ING_RGB8) {
        constexpr bool SW = FMT == ING_RGB8;
        const U32x4A1 u = *reinterpret_cast<const VO_GLOBAL U32x4A1 *>(s);      // bytes 0 .. 15
        const U32x2A1 v = *reinterpret_cast<const VO_GLOBAL U32x2A1 *>(s + 16); // bytes 16 .. 23
        o.a = ing_pack4(ing_gray<SW>(u.a), ing_gray<SW>(alignbyte(u.b, u.a, 3)), ing_gray<SW>(alignbyte(u.c, u.b, 2)),
                        ing_gray<SW>(u.c >> 8));
        o.b = ing_pack4(ing_gray<SW>(u.d), ing_gray<SW>(alignbyte(v.a, u.d, 3)), ing_gray<SW>(alignbyte(v.b, v.a, 2)),
                        ing_gray<SW>(v.b >> 8));
    } else {
        static_assert(FMT == ING_BGRA8 || FMT == ING_RGBA8, "one of the VO_FMT_* formats that need a conversion");
        constexpr bool SW = FMT == ING_RGBA8;
        const U32x4A1 u = *reinterpret_cast<const VO_GLOBAL U32x4A1 *>(s);
        const U32x4A1 v = *reinterpret_cast<const VO_GLOBAL U32x4A1 *>(s + 16);
        o.a = ing_pack4(ing_gray<SW>(u.a), ing_gray<SW>(u.b), ing_gray<SW>(u.c), ing_gray<SW>(u.d));
        o.b = ing_pack4(ing_gray<SW>(v.a), ing_gray<SW>(v.b), ing_gray<SW>(v.c), ing_gray<SW>(v.d));
    }
    return o;
}

// both planes of eight 16-bit words (an interleaved pair, right == left + 1): reads [s, s + 16)
__device__ __forceinline__ void ingest_split8(const VO_GLOBAL uint8_t *__restrict__ s, U32x2A1 &lo, U32x2A1 &hi)
{
    const U32x4A1 u = *reinterpret_cast<const VO_GLOBAL U32x4A1 *>(s);
    lo.a = perm_b32(u.b, u.a, 0x06040200u);
    lo.b = perm_b32(u.d, u.c, 0x06040200u);
    hi.a = perm_b32(u.b, u.a, 0x07050301u);
    hi.b = perm_b32(u.d, u.c, 0x07050301u);
}

// The converting twin of seq_ingest_kernel (seq.hip; the discipline and its reasons are written down there): row r =
// blockIdx.x, + n_waves, ...; image, side, row and both row addresses are wave-uniform; 8 destination pixels per lane.
// SeqIngest.stride is the SOURCE's byte stride (>= w * bpp).
template <int FMT>
__global__ __launch_bounds__(64) void seq_ingest_fmt_kernel(const SeqIngest *__restrict__ tab, int n_rows /* 2 * pairs * h */,
                                                            int n_waves /* = the grid */, int w, int h, int pitch,
                                                            uint8_t *__restrict__ pix0 /* pixel (0,0) of image 0 */, size_t img_bytes)
{
    constexpr int BPP = ingest_bpp(FMT);
    const int last = w - 8; // (w >= 32) the lane that would cross the row end converts the row's last 8 pixels again
    for (int r = blockIdx.x; r < n_rows; r += n_waves) {
        const int img = r / h, row = r - img * h, side = img & 1;
        const SeqIngest e = tab[img >> 1];
        const bool both = FMT == ING_GRAY8_X2 && e.right == e.left + 1; // one interleaved buffer: its left rows write both planes
        if (both && side)
            continue;
        const VO_GLOBAL uint8_t *__restrict__ s = (const VO_GLOBAL uint8_t *)(side ? e.right : e.left) + (size_t)row * e.stride;
        VO_GLOBAL uint8_t *__restrict__ d = (VO_GLOBAL uint8_t *)pix0 + (size_t)(e.image0 + side) * img_bytes + (size_t)row * pitch;
        for (int x0 = 0; x0 < w; x0 += 512) {
            int x = x0 + (int)threadIdx.x * 8;
            if (x < w) {
                x = x < last ? x : last;
                if (both) {
                    U32x2A1 lo, hi;
                    ingest_split8(s + (uint32_t)x * 2u, lo, hi);
                    *reinterpret_cast<VO_GLOBAL U32x2A1 *>(d + (uint32_t)x) = lo;
                    *reinterpret_cast<VO_GLOBAL U32x2A1 *>(d + img_bytes + (uint32_t)x) = hi;
                } else {
                    *reinterpret_cast<VO_GLOBAL U32x2A1 *>(d + (uint32_t)x) = ingest_row8<FMT>(s + (uint32_t)x * (uint32_t)BPP);
                }
            }
        }
    }
}

// The converting twin of pull_image_kernel (pyramid.hip): one image, raw rows with a byte stride (the page-locked staging slot,
// read over PCIe, or a caller's device buffer) -> gray rows at the device pitch.  Wave k of the grid converts 512 pixels of one
// row; like there the call's points and their count ride along: workgroups behind the image's copy n8 float2 from src2 to dst2.
template <int FMT>
__global__ __launch_bounds__(256) void pull_image_fmt_kernel(const uint8_t *__restrict__ src, int src_stride, uint8_t *__restrict__ dst,
                                                             int pitch, int w, int h, uint32_t img_blocks,
                                                             const uint2 *__restrict__ src2, uint2 *__restrict__ dst2, uint32_t n8,
                                                             int *__restrict__ count_dst, int count)
{
    constexpr int BPP = ingest_bpp(FMT);
    if (blockIdx.x < img_blocks) {
        const int chunks = (w + 511) / 512;
        const int wave = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6), row = wave / chunks;
        int x = (wave - row * chunks) * 512 + (int)(threadIdx.x & 63u) * 8;
        if (row < h && x < w) {
            x = x < w - 8 ? x : w - 8;
            const VO_GLOBAL uint8_t *__restrict__ s = (const VO_GLOBAL uint8_t *)src + (size_t)row * src_stride + (uint32_t)x * (uint32_t)BPP;
            *reinterpret_cast<VO_GLOBAL U32x2A1 *>((VO_GLOBAL uint8_t *)dst + (size_t)row * pitch + (uint32_t)x) = ingest_row8<FMT>(s);
        }
    } else {
        const uint32_t i = (blockIdx.x - img_blocks) * 256u + threadIdx.x;
        if (i < n8)
            dst2[i] = src2[i];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && count_dst)
        *count_dst = count;
}

// ONE dispatch over the formats that have kernels here: f(std::integral_constant<int, FMT>) for the format, 0; -1 where there
// is none -- the caller reports it, nothing is copied.  (The launchers below and the CPU emulator's, tests/host_check.)
template <class F>
static int ingest_dispatch(int fmt, F &&f)
{
    switch (fmt) {
    case ING_GRAY8_X2: f(std::integral_constant<int, ING_GRAY8_X2>()); return 0;
    case ING_BGR8: f(std::integral_constant<int, ING_BGR8>()); return 0;
    case ING_RGB8: f(std::integral_constant<int, ING_RGB8>()); return 0;
    case ING_BGRA8: f(std::integral_constant<int, ING_BGRA8>()); return 0;
    case ING_RGBA8: f(std::integral_constant<int, ING_RGBA8>()); return 0;
    }
    return -1;
}

#ifndef VO_HOST_EMUL // (the CPU emulator of tests/host_check launches the kernels above itself)
int launch_seq_ingest_fmt(int fmt, const SeqIngest *tab, int n_pairs, int w, int h, int pitch, uint8_t *pix0, size_t img_bytes,
                          bool over_pcie, hipStream_t stream)
{
    if (n_pairs <= 0)
        return 0;
    const int want = over_pcie ? 192 : 8192; // (launch_seq_ingest's grids, seq.hip)
    const int n_rows = 2 * n_pairs * h;
    const int n_waves = n_rows < want ? n_rows : want;
    return ingest_dispatch(fmt, [&](auto tag) {
        hipLaunchKernelGGL(seq_ingest_fmt_kernel<decltype(tag)::value>, dim3(n_waves), dim3(64), 0, stream, tab, n_rows, n_waves, w, h, pitch,
                           pix0, img_bytes);
    });
}

int launch_pull_image_fmt(int fmt, const void *src, int src_stride, void *dst, int pitch, int w, int h, hipStream_t stream,
                          const void *pts_pinned_dev, void *pts_dst, int n_pts, int *count_dst)
{
    const uint32_t waves = (uint32_t)h * (uint32_t)((w + 511) / 512), img_blocks = (waves + 3) / 4;
    const uint32_t n8 = pts_dst ? (uint32_t)n_pts : 0u;
    return ingest_dispatch(fmt, [&](auto tag) {
        hipLaunchKernelGGL(pull_image_fmt_kernel<decltype(tag)::value>, dim3(img_blocks + (n8 + 255) / 256), dim3(256), 0, stream,
                           (const uint8_t *)src, src_stride, (uint8_t *)dst, pitch, w, h, img_blocks, (const uint2 *)pts_pinned_dev,
                           (uint2 *)pts_dst, n8, count_dst, n_pts);
    });
}
#endif // VO_HOST_EMUL

} // namespace vo
