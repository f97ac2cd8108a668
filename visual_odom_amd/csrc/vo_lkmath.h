// vo_lkmath.h -- packed integer pixel arithmetic of the Lucas-Kanade kernels (lk.hip): the composites over the instruction
// wrappers of vo_isa.h.
//
// OpenCV's LKTrackerInvoker (the arithmetic behind the reference's cv::calcOpticalFlowPyrLK calls,
// feature.cpp:136-139) samples 21 x 21 windows with 14-bit fixed-point bilinear weights:
//     val = DESCALE(p00*iw00 + p01*iw01 + p10*iw10 + p11*iw11, n)        (n = 9 for pixels,
//                                                                         n = 14 for Scharr samples)
// On CDNA4 one lane owns a 7-pixel row segment of the window and evaluates it two pixels at a time
// with the packed 16-bit dot-product instructions:
//   * a pixel pair (p[k], p[k+1]) is lifted out of the 8 loaded bytes with one v_perm_b32 into the
//     HIGH byte of two u16 lanes (= 256 * p), so that v_dot2_u32_u16 against (iw00, iw01) and then
//     (iw10, iw11) yields 256 * S; with the rounding constant 1 << 16 as the initial accumulator the
//     top 16 bits are (S + 256) >> 8, and one packed shift right by 1 gives DESCALE(S, 9) exactly;
//   * the Scharr image is stored pre-multiplied by 4 (|4 d| <= 16320 fits int16), so two
//     v_dot2_i32_i16 with initial accumulator 1 << 15 leave DESCALE(S, 14) in the top 16 bits;
//   * results are re-packed two per register (v_perm_b32) so that diff = val - I is one v_pk_sub_i16
//     and b1 += diff*Ix, b2 += diff*Iy are one v_dot2_i32_i16 each per pixel pair.
//   * the one-feature kernels group the same four products by COLUMN (lift8_cols / blend7_cols /
//     bilinear7_deriv_cols below): vertical pairs (t[k], b[k]) against (iw00, iw10) and (iw01, iw11), so that
//     every column is lifted once; the horizontal composites stay for the pair kernel of the developer build and
//     as the statement the vertical ones are tested against (tests/host_check/lk_cols_cases.h).
// Every step is exact integer arithmetic, so the result is bit-identical to the scalar formula.  The
// host build of this header (tests/test_device_math_on_host.py) shows that for the `#else` text of the
// wrappers (vo_isa.h); tests/test_gpu_device_units.py runs the instructions themselves on gfx950, every
// wrapper and every composite, against that host text and the plain restatement.
#pragma once

#include "vo_isa.h" // the instruction wrappers (device: the CDNA4 instruction; host: its definition) and VO_HD

#include <math.h>

namespace vo {

VO_HD uint32_t f32_bits(float v)
{
    uint32_t u;
    __builtin_memcpy(&u, &v, 4);
    return u;
}

// ---- selectors ------------------------------------------------------------------------------------
// bytes k and k+1 of the 8 loaded bytes into the high byte of the two u16 lanes (256*p[k], 256*p[k+1])
#define VO_SEL_PIX(k) (0x0cu | ((uint32_t)(k) << 8) | (0x0cu << 16) | ((uint32_t)((k) + 1) << 24))
constexpr uint32_t VO_SEL_LO16 = 0x05040100u; // (lo.lo16, hi.lo16)
constexpr uint32_t VO_SEL_HI16 = 0x07060302u; // (lo.hi16, hi.hi16)

// two weights as int16 lanes (|w| <= 2^14, so v_cvt_pk_i16_i32's saturation never triggers)
VO_HD uint32_t pack_w(int w_lo, int w_hi)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pk_i16(w_lo, w_hi));
#else
    return (uint32_t)(w_lo & 0xffff) | ((uint32_t)w_hi << 16);
#endif
}

// ---- the bilinear weights ------------------------------------------------------------------------
// 14-bit fixed-point bilinear weights of OpenCV's LKTrackerInvoker from the fractional parts of the
// window corner: iw00 = cvRound((1-a)*(1-b)*2^14), iw01 = cvRound(a*(1-b)*2^14), iw10 = cvRound((1-a)*b*2^14),
// iw11 = 2^14 - iw00 - iw01 - iw10, returned as packed int16 pairs: by row, wt = (iw00, iw01), wb = (iw10, iw11)
// (lk_weights: the samplers over horizontal pixel pairs), or by column, wl = (iw00, iw10), wr = (iw01, iw11)
// (lk_weights_cols: the samplers over vertical pairs below) -- the two differ in the packing selectors' operands only.
//   * the scale is folded in exactly (a power of two, see below);
//   * cvRound (round half to even) = adding 1.5 * 2^23: the f32 sum has ulp 1, so the add rounds the
//     product to the nearest-even integer and leaves it in the low mantissa bits.  The raw bit patterns
//     are packed / summed directly (0x4B400000 has no low 16 bits), no v_rndne / v_cvt per weight.
constexpr int LK_W_BITS = 14;
// x * s + m on both lanes with ONE rounding each: v_pk_fma_f32
typedef float F32x2 __attribute__((vector_size(8)));
VO_HD F32x2 pk_fma_f32(F32x2 x, float s, float m)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const F32x2 sv = {s, s}, mv = {m, m};
    return __builtin_elementwise_fma(x, sv, mv);
#else
    const F32x2 r = {fmaf(x[0], s, m), fmaf(x[1], s, m)};
    return r;
#endif
}
template <bool COLS>
VO_HD void lk_weights_packed(float a, float b, uint32_t &w0, uint32_t &w1)
{
    const float s = (float)(1 << LK_W_BITS), magic = 12582912.f; // 1.5 * 2^23 = 0x4B400000
    // Written on pairs, the way the packed f32 instructions take them: (a1, b1) = 1 - (a, b) is one subtraction, (a * b1, b * a1)
    // one multiply of the pair with the swapped one, and that pair goes into the packed scale-and-round AS IT IS -- (iw01, iw10) --
    // beside a plain multiply for a1 * b1.  (Pairing a1 * b1 with one of the two put a register copy between the multiplies and
    // the fused multiply-add, profiles/r12_lk_iteration_branches.md; the three products, their operands and their roundings are
    // what they were.)  The scale moves behind the product -- a power of two goes through a
    // rounded product unchanged, fl((a1 * s) * b1) == fl(a1 * b1) * s, and where the product underflows both forms vanish in the
    // sum -- so "* s + magic" is one fused multiply-add with an exact product: one rounding, the one the add always had.
    const F32x2 p = {a, b}, q = 1.f - p, qswap = {q[1], q[0]};
    const F32x2 r = pk_fma_f32(p * qswap, s, magic); // of (a * b1, b * a1)
    const uint32_t r00 = f32_bits(fmaf(q[0] * q[1], s, magic));
    const uint32_t r01 = f32_bits(r[0]), r10 = f32_bits(r[1]);
    // iw11 = 2^14 - (r00 + r01 + r10 - 3 * 0x4B400000)   (mod 2^32)
    const uint32_t iw11 = ((1u << LK_W_BITS) + 3u * 0x4B400000u) - (r00 + r01 + r10);
    w0 = perm_b32(COLS ? r10 : r01, r00, VO_SEL_LO16);
    w1 = perm_b32(iw11, COLS ? r01 : r10, VO_SEL_LO16); // signed lanes: iw11 may be -1
}
VO_HD void lk_weights(float a, float b, uint32_t &wt, uint32_t &wb)
{
    lk_weights_packed<false>(a, b, wt, wb);
}
VO_HD void lk_weights_cols(float a, float b, uint32_t &wl, uint32_t &wr)
{
    lk_weights_packed<true>(a, b, wl, wr);
}

// ---- one 7-pixel row segment ----------------------------------------------------------------------
// t = bytes x..x+7 of the upper image row, b = the same columns one row below.
// wt = (iw00, iw01), wb = (iw10, iw11) as packed int16 lanes.
// out[m] = (val[2m], val[2m+1]) as packed int16, out[3].hi = 0;
// val[k] = DESCALE(t[k]*iw00 + t[k+1]*iw01 + b[k]*iw10 + b[k+1]*iw11, 9).
// iw00, iw01, iw10 are rounded non-negative products, but iw11 = 2^14 - (their sum) is -1 when the
// three roundings add up to 2^14 + 1; an unsigned dot product cannot carry a negative weight, so
// that (rare, wave-uniform) case zeroes the weight and subtracts |iw11| * 256*p11 explicitly.
VO_HD void bilinear7_u8(uint32_t t_lo, uint32_t t_hi, uint32_t b_lo, uint32_t b_hi, uint32_t wt, uint32_t wb,
                        uint32_t out[4])
{
    uint32_t acc[8];
    if (!(wb & 0x80000000u)) {
#define VO_PIX_STEP(k)                                                                               \
    acc[k] = udot2(perm_b32(b_hi, b_lo, VO_SEL_PIX(k)), wb,                                          \
                   udot2(perm_b32(t_hi, t_lo, VO_SEL_PIX(k)), wt, 1u << 16));
        VO_PIX_STEP(0) VO_PIX_STEP(1) VO_PIX_STEP(2) VO_PIX_STEP(3) VO_PIX_STEP(4) VO_PIX_STEP(5) VO_PIX_STEP(6)
#undef VO_PIX_STEP
    } else {
        const uint32_t wb0 = wb & 0xffffu, kneg = (uint32_t)(-(int32_t)((int16_t)(wb >> 16)));
#define VO_PIX_STEP(k)                                                                               \
    {                                                                                                \
        const uint32_t pb = perm_b32(b_hi, b_lo, VO_SEL_PIX(k));                                     \
        acc[k] = udot2(pb, wb0, udot2(perm_b32(t_hi, t_lo, VO_SEL_PIX(k)), wt, 1u << 16)) -          \
                 kneg * (pb >> 16);                                                                  \
    }
        VO_PIX_STEP(0) VO_PIX_STEP(1) VO_PIX_STEP(2) VO_PIX_STEP(3) VO_PIX_STEP(4) VO_PIX_STEP(5) VO_PIX_STEP(6)
#undef VO_PIX_STEP
    }
    acc[7] = 0;
#pragma unroll
    for (int m = 0; m < 4; m++)
        out[m] = pk_lshr1_u16(perm_b32(acc[2 * m + 1], acc[2 * m], VO_SEL_HI16));
}

// The same in two steps, for callers that sample one pixel cell several times with different weights:
// lift7 does the weight-independent part (the 7 pixel pairs of one row as u16 lanes 256*p[k], 256*p[k+1]),
// blend7 the weighted sum.  blend7(lift7(top), lift7(bottom)) == bilinear7_u8.
VO_HD void lift7(uint32_t lo, uint32_t hi, uint32_t pair[7])
{
#define VO_LIFT(k) pair[k] = perm_b32(hi, lo, VO_SEL_PIX(k));
    VO_LIFT(0) VO_LIFT(1) VO_LIFT(2) VO_LIFT(3) VO_LIFT(4) VO_LIFT(5) VO_LIFT(6)
#undef VO_LIFT
}

VO_HD void blend7(const uint32_t pt[7], const uint32_t pb[7], uint32_t wt, uint32_t wb, uint32_t out[4])
{
    uint32_t acc[8];
    if (!(wb & 0x80000000u)) {
#pragma unroll
        for (int k = 0; k < 7; k++)
            acc[k] = udot2(pb[k], wb, udot2(pt[k], wt, 1u << 16));
    } else {
        const uint32_t wb0 = wb & 0xffffu, kneg = (uint32_t)(-(int32_t)((int16_t)(wb >> 16)));
#pragma unroll
        for (int k = 0; k < 7; k++)
            acc[k] = udot2(pb[k], wb0, udot2(pt[k], wt, 1u << 16)) - kneg * (pb[k] >> 16);
    }
    acc[7] = 0;
#pragma unroll
    for (int m = 0; m < 4; m++)
        out[m] = pk_lshr1_u16(perm_b32(acc[2 * m + 1], acc[2 * m], VO_SEL_HI16));
}

// ---- the same samples from VERTICAL pairs --------------------------------------------------------
// The four products of a sample can be grouped by column instead of by row:
//     S[k] = dot2((t[k], b[k]), (iw00, iw10)) + dot2((t[k+1], b[k+1]), (iw01, iw11))
// so the 8 columns of a segment are lifted ONCE each as (256*t[k], 256*b[k]) -- one v_perm_b32 of the two loaded dwords
// that hold column k -- where the horizontal form lifts every inner column twice (14 pairs).  The weights go in as
// wl = (iw00, iw10), wr = (iw01, iw11); the 14 dot products, their order and every partial sum's range are the same, and
// so is every result, bit for bit.  lk.hip's one-feature kernels sample through these.
// byte k (0..3) of `lo` and of `hi` into the high byte of the two u16 lanes: (256*lo[k], 256*hi[k])
#define VO_SEL_COL(k) (0x0cu | ((uint32_t)(k) << 8) | (0x0cu << 16) | ((uint32_t)((k) + 4) << 24))
VO_HD void lift8_cols(uint32_t t_lo, uint32_t t_hi, uint32_t b_lo, uint32_t b_hi, uint32_t col[8])
{
#define VO_LIFT(k) col[k] = perm_b32(b_lo, t_lo, VO_SEL_COL(k)), col[(k) + 4] = perm_b32(b_hi, t_hi, VO_SEL_COL(k));
    VO_LIFT(0) VO_LIFT(1) VO_LIFT(2) VO_LIFT(3)
#undef VO_LIFT
}

// blend7_cols(lift8_cols(t, b), wl, wr) == bilinear7_u8(t, b, wt, wb).  iw11 = -1 is the high lane of wr: that case
// zeroes the weight and subtracts |iw11| * 256*b[k+1], the high lane of column k + 1.
VO_HD void blend7_cols(const uint32_t col[8], uint32_t wl, uint32_t wr, uint32_t out[4])
{
    uint32_t acc[7];
    if (!(wr & 0x80000000u)) {
#pragma unroll
        for (int k = 0; k < 7; k++)
            acc[k] = udot2(col[k + 1], wr, udot2(col[k], wl, 1u << 16));
    } else {
        const uint32_t wr0 = wr & 0xffffu, kneg = (uint32_t)(-(int32_t)((int16_t)(wr >> 16)));
#pragma unroll
        for (int k = 0; k < 7; k++) {
            uint32_t c = col[k + 1];
#if defined(__HIP_DEVICE_COMPILE__)
            // the shift below depends on the column only: seen through, it is hoisted out of a caller's loop over weights
            // into the code that lifts the columns, i.e. from the rare case into the common one
            asm volatile("" : "+v"(c));
#endif
            acc[k] = udot2(c, wr0, udot2(col[k], wl, 1u << 16)) - kneg * (c >> 16);
        }
    }
#pragma unroll
    for (int m = 0; m < 3; m++)
        out[m] = pk_lshr1_u16(perm_b32(acc[2 * m + 1], acc[2 * m], VO_SEL_HI16));
    // (val[6], 0): the high half of acc[6], shifted once more, is the whole word shifted right by 17 -- one instruction for two, and
    // no selector beside a zero, which the compiler keeps in a vector register of its own for the whole kernel
    out[3] = acc[6] >> 17;
}

// The same for a caller that knows the sign of iw11 as a wave-uniform value (`neg`; lk.hip's iteration reads it off the packed
// weight through v_readfirstlane_b32): one scalar compare-and-branch, where the test of `wr` -- a value per lane -- is compiled as
// a divergent region that saves, rewrites and restores the execution mask in every call although all lanes agree.  The first
// links of the seven chains do not depend on the case and stand in front of the branch; the rare case is kept out of line.
VO_HD void blend7_cols(const uint32_t col[8], uint32_t wl, uint32_t wr, bool neg, uint32_t out[4])
{
    uint32_t acc[7];
#pragma unroll
    for (int k = 0; k < 7; k++)
        acc[k] = udot2(col[k], wl, 1u << 16);
    if (__builtin_expect(neg, 0)) {
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" ::: "memory"); // keep the rare case out of the common path
#endif
        const uint32_t wr0 = wr & 0xffffu, kneg = (uint32_t)(-(int32_t)((int16_t)(wr >> 16)));
#pragma unroll
        for (int k = 0; k < 7; k++) {
            uint32_t c = col[k + 1];
#if defined(__HIP_DEVICE_COMPILE__)
            asm volatile("" : "+v"(c)); // (as above: the shift stays in the rare case)
#endif
            acc[k] = udot2(c, wr0, acc[k]) - kneg * (c >> 16);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 7; k++)
            acc[k] = udot2(col[k + 1], wr, acc[k]);
    }
#pragma unroll
    for (int m = 0; m < 3; m++)
        out[m] = pk_lshr1_u16(perm_b32(acc[2 * m + 1], acc[2 * m], VO_SEL_HI16));
    out[3] = acc[6] >> 17; // (val[6], 0): the high half of acc[6], shifted once more, is the whole word shifted -- no selector
}

VO_HD void bilinear7_u8_cols(uint32_t t_lo, uint32_t t_hi, uint32_t b_lo, uint32_t b_hi, uint32_t wl, uint32_t wr,
                             uint32_t out[4])
{
    uint32_t col[8];
    lift8_cols(t_lo, t_hi, b_lo, b_hi, col);
    blend7_cols(col, wl, wr, out);
}

// Scharr samples: d[k] = (4*Ix | 4*Iy << 16) of pixel x+k, rows top / bottom, k = 0..7.
// ix[m] = (Ixval[2m], Ixval[2m+1]), iy likewise; *val[k] = DESCALE(sum d*iw, 14) of the true derivative.
VO_HD void bilinear7_deriv(const uint32_t dt[8], const uint32_t db[8], uint32_t wt, uint32_t wb, uint32_t ix[4],
                           uint32_t iy[4])
{
    int32_t ax[8], ay[8];
#pragma unroll
    for (int k = 0; k < 7; k++) {
        ax[k] = sdot2(perm_b32(db[k + 1], db[k], VO_SEL_LO16), wb,
                      sdot2_first(perm_b32(dt[k + 1], dt[k], VO_SEL_LO16), wt, 1 << 15));
        ay[k] = sdot2(perm_b32(db[k + 1], db[k], VO_SEL_HI16), wb,
                      sdot2_first(perm_b32(dt[k + 1], dt[k], VO_SEL_HI16), wt, 1 << 15));
    }
    ax[7] = ay[7] = 0;
#pragma unroll
    for (int m = 0; m < 4; m++) {
        ix[m] = perm_b32((uint32_t)ax[2 * m + 1], (uint32_t)ax[2 * m], VO_SEL_HI16);
        iy[m] = perm_b32((uint32_t)ay[2 * m + 1], (uint32_t)ay[2 * m], VO_SEL_HI16);
    }
}

// bilinear7_deriv on (wl, wr): column k regrouped as (Ix_t[k], Ix_b[k]) and (Iy_t[k], Iy_b[k]), 16 v_perm_b32 for 28
VO_HD void bilinear7_deriv_cols(const uint32_t dt[8], const uint32_t db[8], uint32_t wl, uint32_t wr, uint32_t ix[4],
                                uint32_t iy[4])
{
    uint32_t cx[8], cy[8];
    int32_t ax[8], ay[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        cx[k] = perm_b32(db[k], dt[k], VO_SEL_LO16);
        cy[k] = perm_b32(db[k], dt[k], VO_SEL_HI16);
    }
#pragma unroll
    for (int k = 0; k < 7; k++) {
        ax[k] = sdot2(cx[k + 1], wr, sdot2_first(cx[k], wl, 1 << 15));
        ay[k] = sdot2(cy[k + 1], wr, sdot2_first(cy[k], wl, 1 << 15));
    }
    ax[7] = ay[7] = 0;
#pragma unroll
    for (int m = 0; m < 4; m++) {
        ix[m] = perm_b32((uint32_t)ax[2 * m + 1], (uint32_t)ax[2 * m], VO_SEL_HI16);
        iy[m] = perm_b32((uint32_t)ay[2 * m + 1], (uint32_t)ay[2 * m], VO_SEL_HI16);
    }
}

// ---- do the iteration's two sums fit 32 bits? -------------------------------------------------------
// b1 = sum (Jp - Ip) * Ixp and b2 = sum (Jp - Ip) * Iyp over the window can reach 2^34 in general, which is what
// wave_sum2_exact_f32's two halves are for.  For most templates they cannot, and the level's structure tensor says so:
//   * Jp and Ip are DESCALE(sum of p * iw, 9) of pixels p in [0, 255] under weights that sum to 2^14, three of them >= 0 and
//     iw11 >= -1: both lie in [0, 8160] (iw11 = -1: at most (255 * (2^14 + 1) + 256) >> 9 = 8160, at least (-255 + 256) >> 9 = 0),
//     so |Jp - Ip| <= 8160 < 2^13 whatever J holds;
//   * Cauchy-Schwarz over the n <= 441 pixels of the window: sum |Ixp| <= sqrt(n * sum Ixp^2) = sqrt(n * A11raw);
//   * hence |b1| <= 2^13 * 21 * sqrt(A11raw), which is < 2^31 for A11raw < (2^18 / 21)^2 = 1.558e8 (1.569e8 with 8160).
// A11raw, A22raw: the exact integer sums of wave_sum3_exact_f32 rounded once to f32 (relative error 2^-24), BEFORE the 2^-20
// of FLT_SCALE.  The threshold 1.5e8 leaves 3.7 % for that rounding and holds for every window of 21 x 21 and below (a smaller n
// only lowers the bound).  Written on the bit patterns -- non-negative floats order like their bits, a negative value or a NaN
// reads as "does not fit" -- so that on the device, where both sums sit in scalar registers, the test is s_max_u32 + s_cmp_lt_u32.
constexpr float LK_FIT_RAW_MAX = 1.5e8f;
constexpr uint32_t LK_FIT_RAW_MAX_BITS = 0x4D0F0D18u; // of 1.5e8f (tests/host_check/lk_fit_host.cpp holds the two together)
VO_HD bool lk_sums_fit(float a11_raw, float a22_raw)
{
    const uint32_t u = f32_bits(a11_raw), v = f32_bits(a22_raw);
    return (u > v ? u : v) < LK_FIT_RAW_MAX_BITS;
}

// Scharr 3x3 (cv::calcSharrDeriv) of the centre pixel of a 3x3 patch, stored pre-multiplied by 4
VO_HD uint32_t scharr4_packed(int p00, int p01, int p02, int p10, int p12, int p20, int p21, int p22)
{
    // t0(x) = (row-1 + row+1)*3 + row*10 ; t1(x) = row+1 - row-1 ; Ix = t0(x+1) - t0(x-1) ;
    // Iy = (t1(x+1) + t1(x-1))*3 + t1(x)*10
    int ix = ((p02 + p22) * 3 + p12 * 10) - ((p00 + p20) * 3 + p10 * 10);
    int iy = ((p22 - p02) + (p20 - p00)) * 3 + (p21 - p01) * 10;
    return ((uint32_t)(ix * 4) & 0xffffu) | ((uint32_t)(iy * 4) << 16);
}

} // namespace vo
