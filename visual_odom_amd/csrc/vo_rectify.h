// vo_rectify.h -- stereo rectification at ingest (vo_params.rectify, include/vo_hip.h): what the host (vo_set_params packs the
// caller's maps), the device (rectify.hip) and the CPU emulator (tests/host_check/rectify_emu.cpp) share -- the packed map, the
// geometry of a raw plane, and the per-pixel formula.
//
// SEMANTICS: cv::remap(src, dst, map_x, map_y, INTER_LINEAR, BORDER_CONSTANT, 0) for CV_8UC1 with CV_32FC1 maps in OpenCV's
// fixed-point form (INTER_BITS = 5 for the coordinates, INTER_REMAP_COEF_BITS = 15 for the weights).  Destination pixel (x, y):
//   sx = rint_half_even(map_x[y][x] * 32)   sy = rint_half_even(map_y[y][x] * 32)       (x 32 is exact in f32)
//   ix = sx >> 5, a = sx & 31               iy = sy >> 5, b = sy & 31                   (arithmetic shift)
//   p(j, i) = src[j][i] inside the image, 0 outside
//   dst = ((32-a)(32-b) p(iy,ix) + a(32-b) p(iy,ix+1) + (32-a) b p(iy+1,ix) + a b p(iy+1,ix+1) + 512) >> 10
// OpenCV's table holds the 15-bit weights round(32768 * wa * wb) with wa, wb multiples of 1/32: every one of them is exactly 32
// times the product above (products of two 5-bit fractions need 10 bits), so (sum w15 p + 16384) >> 15 is the line above.  A
// non-finite entry, or one whose ix / iy leaves int16 (x86 cvRound gives INT_MIN, saturate_cast<short> pins it), has all four
// taps outside and gives 0.
//
// PACKED MAP: one dword per destination pixel, (sx - 32 x) as the low i16 and (sy - 32 y) as the high i16 -- displacements up
// to +-1023 pixels -- and ONE reserved pattern, RECT_OUTSIDE, for "all four taps outside" (whatever the entry was).  A larger
// displacement whose taps are not all outside cannot be packed: rect_pack reports it and vo_set_params returns VO_ERR_ARG.
//
// RAW PLANE: what the ingest of a rectifying context writes instead of level 0 -- the w x h gray image at pitch
// rect_raw_pitch(w) inside a frame of zeros at least RECT_FRAME pixels wide on every side, written once at allocation (ingest
// writes the interior, and zeros where its contiguous copy runs over the columns between two rows).  With ix clamped to
// [-2, w] and iy to [-2, h] every tap is a read inside the plane and an outside tap reads 0: the border costs no predicate.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "vo_isa.h" // udot4

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif

namespace vo {

constexpr uint32_t RECT_OUTSIDE = 0x80008000u; // (displacements of -32768 / 32 pixels are never packed)
constexpr int RECT_FRAME = 2;
constexpr int RECT_MAX_DISP = 1023 * 32; // |sx - 32 x|, |sy - 32 y| of a packed entry

// bytes between the rows of a raw plane (a multiple of 16, >= w + 2 * RECT_FRAME), offset of pixel (0, 0) (16-byte aligned:
// the gray pull kernel stores 16 bytes at a time) and size of the plane: rows -2 .. h + 1, columns -2 .. w + 1 lie inside
__host__ __device__ constexpr int rect_raw_pitch(int w) { return (w + 2 * RECT_FRAME + 15) / 16 * 16; }
__host__ __device__ constexpr size_t rect_raw_origin(int w) { return (size_t)RECT_FRAME * rect_raw_pitch(w) + 16; }
__host__ __device__ constexpr size_t rect_raw_bytes(int w, int h) { return (size_t)rect_raw_pitch(w) * (h + 2 * RECT_FRAME) + 32; }

// one map coordinate in 1/32 pixel; false: non-finite, or its integer part leaves int16 (all taps outside)
inline bool rect_fix(float m, int *s)
{
    const float v = m * 32.0f;
    if (!(fabsf(v) < 1048576.0f)) // (NaN, inf and everything beyond +-32768 pixels)
        return false;
    *s = (int)nearbyintf(v); // the default rounding mode: to nearest, ties to even (cvRound on x86)
    const int i = *s >> 5;
    return i >= -32768 && i <= 32767;
}

// the packed entry of destination pixel (x, y) of a w x h image; false: a displacement beyond RECT_MAX_DISP that is not wholly outside
inline bool rect_pack(float mx, float my, int x, int y, int w, int h, uint32_t *out)
{
    int sx, sy;
    *out = RECT_OUTSIDE;
    if (!rect_fix(mx, &sx) || !rect_fix(my, &sy))
        return true;
    const int ix = sx >> 5, iy = sy >> 5;
    if (ix < -1 || ix >= w || iy < -1 || iy >= h) // taps ix, ix + 1 and iy, iy + 1
        return true;
    const int dx = sx - 32 * x, dy = sy - 32 * y;
    if (dx < -RECT_MAX_DISP || dx > RECT_MAX_DISP || dy < -RECT_MAX_DISP || dy > RECT_MAX_DISP)
        return false;
    *out = ((uint32_t)dx & 0xffffu) | ((uint32_t)dy << 16);
    return true;
}

// where the taps of a packed entry lie and how they are weighted: the entry of destination pixel (x, y)
struct RectTap {
    int ix, iy;    // top-left tap, clamped to [-2, w] x [-2, h]
    uint32_t wx, b; // (32 - a) | a << 8: the weights of the two bytes of a row; b
};
__host__ __device__ inline RectTap rect_tap(uint32_t m, int x, int y, int w, int h)
{
    const int sx = 32 * x + (int)(int16_t)(m & 0xffffu), sy = 32 * y + (int)(int16_t)(m >> 16);
    int ix = sx >> 5, iy = sy >> 5;
    const uint32_t a = (uint32_t)sx & 31u;
    ix = m == RECT_OUTSIDE ? -RECT_FRAME : ix;
    RectTap t;
    t.ix = ix < -RECT_FRAME ? -RECT_FRAME : ix > w ? w : ix;
    t.iy = iy < -RECT_FRAME ? -RECT_FRAME : iy > h ? h : iy;
    t.wx = (32u - a) | (a << 8);
    t.b = (uint32_t)sy & 31u;
    return t;
}
// row0 / row1: the two bytes at (iy, ix), (iy, ix + 1) and at (iy + 1, ix), (iy + 1, ix + 1) as the low halves of a dword.
// Horizontal first (v_dot4_u32_u8): h0, h1 <= 32 * 255 = 8160; the sum <= 32 * 8160 + 512.
__host__ __device__ inline uint32_t rect_blend(uint32_t row0, uint32_t row1, uint32_t wx, uint32_t b)
{
    const uint32_t h0 = udot4(row0, wx, 0u), h1 = udot4(row1, wx, 0u);
    return (h0 * (32u - b) + h1 * b + 512u) >> 10;
}

} // namespace vo
