// unit_cases.h -- TEST ONLY.  One entry point per routine of the VO_HD device-math headers, in a form that g++
// (host_check.cpp: hc_case), the host pass of hipcc (device_check.hip --host) and gfx950 (device_check.hip: one thread per
// case) all compile from this one text: a case is IN bytes of operands -> OUT bytes of results, both raw little-endian
// records whose fields sit at their natural alignment.  No references and no judgement here: tests/test_gpu_device_units.py
// and tests/test_device_check_host_mode.py compare the three builds bit for bit.  Not a product path.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../visual_odom_amd/csrc/vo_epnp.h"
#include "../../visual_odom_amd/csrc/vo_fivept.h"
#include "../../visual_odom_amd/csrc/vo_linalg.h"
#include "../../visual_odom_amd/csrc/vo_lkmath.h"
#include "../../visual_odom_amd/csrc/vo_p3p.h"
#include "../../visual_odom_amd/csrc/vo_tri.h"

#if defined(__HIPCC__)
#define UC_HD __host__ __device__ __forceinline__
#else
#define UC_HD inline
#endif

namespace uc {

// ---- vo_math.h: f64 x -> f64 y.  W = 0 cbrt, 1 acos, 2 cos, 3 sin, 4 vo_lm_lambda((int)x)
constexpr const char *math_name(int w)
{
    return w == 0 ? "math_cbrt" : w == 1 ? "math_acos" : w == 2 ? "math_cos" : w == 3 ? "math_sin" : "math_lambda";
}
template <int W>
struct Math {
    static constexpr int IN = 8, OUT = 8;
    static constexpr const char *name() { return math_name(W); }
    static UC_HD void run(const void *in, void *out)
    {
        const double x = *(const double *)in;
        *(double *)out = W == 0 ? vo::vo_cbrt(x) : W == 1 ? vo::vo_acos(x) : W == 2 ? vo::vo_cos(x) : W == 3 ? vo::vo_sin(x)
                                                                                                           : vo::vo_lm_lambda((int)x);
    }
};

// ---- pose headers
// f32 xyz[15], uv[10], K[9] -> f64 rvec[3], tvec[3]
struct Epnp5 {
    static constexpr int IN = 34 * 4, OUT = 6 * 8;
    static constexpr const char *name() { return "epnp5"; }
    static UC_HD void run(const void *in, void *out)
    {
        const float *f = (const float *)in;
        double *o = (double *)out;
        vo::epnp5_solve(f, f + 15, f + 25, o, o + 3);
    }
};
// f32 xyz[12], uv[8], K[9] -> f64 number of solutions, rvec[3], tvec[3] of the first sorted one (zeros when there is none)
struct P3p4 {
    static constexpr int IN = 29 * 4, OUT = 7 * 8;
    static constexpr const char *name() { return "p3p4"; }
    static UC_HD void run(const void *in, void *out)
    {
        const float *f = (const float *)in;
        double *o = (double *)out;
        for (int k = 1; k < 7; k++)
            o[k] = 0;
        o[0] = (double)vo::p3p4_solve(f, f + 12, f + 20, o + 1, o + 4);
    }
};
// f64 a, b, c, d, e -> f64 number of real roots, x[4] (zeros beyond the count the routine wrote)
struct P3pDeg4 {
    static constexpr int IN = 5 * 8, OUT = 5 * 8;
    static constexpr const char *name() { return "p3p_deg4"; }
    static UC_HD void run(const void *in, void *out)
    {
        const double *c = (const double *)in;
        double *o = (double *)out;
        for (int k = 1; k < 5; k++)
            o[k] = 0;
        o[0] = (double)vo::p3p_deg4(c[0], c[1], c[2], c[3], c[4], o + 1);
    }
};
// f64 rvec[3] -> f64 R[9], J[27]
struct RodV2m {
    static constexpr int IN = 3 * 8, OUT = 36 * 8;
    static constexpr const char *name() { return "rodrigues_v2m"; }
    static UC_HD void run(const void *in, void *out) { vo::rodrigues_v2m((const double *)in, (double *)out, (double *)out + 9); }
};
// f64 R[9] -> f64 rvec[3]
struct RodM2v {
    static constexpr int IN = 9 * 8, OUT = 3 * 8;
    static constexpr const char *name() { return "rodrigues_m2v"; }
    static UC_HD void run(const void *in, void *out) { vo::rodrigues_m2v((const double *)in, (double *)out); }
};
// f32 Pl[12], Pr[12], xl, yl, xr, yr -> f32 xyz[3]
struct Triangulate {
    static constexpr int IN = 28 * 4, OUT = 3 * 4;
    static constexpr const char *name() { return "triangulate"; }
    static UC_HD void run(const void *in, void *out)
    {
        const float *f = (const float *)in;
        vo::triangulate_one(f, f + 12, f[24], f[25], f[26], f[27], (float *)out);
    }
};
// f64 q1[10], q2[10] -> f64 number of models, Es[10][9] (zeros beyond the count)
struct FivePoint {
    static constexpr int IN = 20 * 8, OUT = 91 * 8;
    static constexpr const char *name() { return "five_point"; }
    static UC_HD void run(const void *in, void *out)
    {
        const double *q = (const double *)in;
        double *o = (double *)out;
        double Es[90];
        for (int k = 0; k < 90; k++)
            Es[k] = 0;
        const int n = vo::five_point_solve(q, q + 10, Es);
        o[0] = (double)n;
        for (int k = 0; k < 90; k++)
            o[1 + k] = k < 9 * n ? Es[k] : 0.0;
    }
};
// f64 E[9], x1x, x1y, x2x, x2y -> f32
struct Sampson {
    static constexpr int IN = 13 * 8, OUT = 4;
    static constexpr const char *name() { return "sampson"; }
    static UC_HD void run(const void *in, void *out)
    {
        const double *d = (const double *)in;
        *(float *)out = vo::em_sampson_error(d, d[9], d[10], d[11], d[12]);
    }
};
// f64 E[9] -> f64 R1[9], R2[9], t[3]
struct Decompose {
    static constexpr int IN = 9 * 8, OUT = 21 * 8;
    static constexpr const char *name() { return "decompose"; }
    static UC_HD void run(const void *in, void *out)
    {
        double *o = (double *)out;
        vo::em_decompose((const double *)in, o, o + 9, o + 18);
    }
};
// f64 P[12], x0, y0, x1, y1, dist -> i32 0 / 1
struct Cheirality {
    static constexpr int IN = 17 * 8, OUT = 4;
    static constexpr const char *name() { return "cheirality"; }
    static UC_HD void run(const void *in, void *out)
    {
        const double *d = (const double *)in;
        *(int32_t *)out = vo::em_cheirality(d, d[12], d[13], d[14], d[15], d[16]) ? 1 : 0;
    }
};
// f64 A[36] row-major, b[6] -> f64 x[6]
struct Solve6 {
    static constexpr int IN = 42 * 8, OUT = 6 * 8;
    static constexpr const char *name() { return "solve6"; }
    static UC_HD void run(const void *in, void *out)
    {
        const double *d = (const double *)in;
        vo::solve_svd<6, 6>(d, d + 36, (double *)out);
    }
};
// f64 At[144] -> f64 sorted, normalised rows[144], singular values[12]: the one-lane routine of the monolithic EPnP kernel
struct Svd12 {
    static constexpr int IN = 144 * 8, OUT = 156 * 8;
    static constexpr const char *name() { return "svd12"; }
    static UC_HD void run(const void *in, void *out)
    {
        double *o = (double *)out;
        for (int k = 0; k < 144; k++)
            o[k] = ((const double *)in)[k];
        vo::jacobi_svd<12, 12, false, 1>(o, o + 144, nullptr);
    }
};

// ---- vo_isa.h (and pack_w of vo_lkmath.h), the raw instruction wrappers: u32 a, b, c -> u32
constexpr const char *lk_raw_name(int w)
{
    return w == 0    ? "lk_perm_b32"
           : w == 1  ? "lk_udot2"
           : w == 2  ? "lk_sdot2"
           : w == 3  ? "lk_sdot2_first"
           : w == 4  ? "lk_pk_sub_i16"
           : w == 5  ? "lk_pk_lshr1_u16"
           : w == 6  ? "lk_udot4"
           : w == 7  ? "lk_pk_add_u16"
           : w == 8  ? "lk_pk_subsat_u16"
           : w == 9  ? "lk_pk_min_u16"
           : w == 10 ? "lk_pk_mad_u16"
           : w == 11 ? "lk_alignbyte"
           : w == 12 ? "lk_pack_w"
                     : "lk_pk_absdiff_i16";
}
template <int W>
struct LkRaw {
    static constexpr int IN = 12, OUT = 4;
    static constexpr const char *name() { return lk_raw_name(W); }
    static UC_HD void run(const void *in, void *out)
    {
        const uint32_t a = ((const uint32_t *)in)[0], b = ((const uint32_t *)in)[1], c = ((const uint32_t *)in)[2];
        *(uint32_t *)out = W == 0    ? vo::perm_b32(a, b, c) // (hi, lo, selector)
                           : W == 1  ? vo::udot2(a, b, c)
                           : W == 2  ? (uint32_t)vo::sdot2(a, b, (int32_t)c)
                           : W == 3  ? (uint32_t)vo::sdot2_first(a, b, (int32_t)c)
                           : W == 4  ? vo::pk_sub_i16(a, b)
                           : W == 5  ? vo::pk_lshr1_u16(a)
                           : W == 6  ? vo::udot4(a, b, c)
                           : W == 7  ? vo::pk_add_u16(a, b)
                           : W == 8  ? vo::pk_subsat_u16(a, b)
                           : W == 9  ? vo::pk_min_u16(a, b)
                           : W == 10 ? vo::pk_mad_u16(a, b, c)
                           : W == 11 ? vo::alignbyte(a, b, c)
                           : W == 12 ? vo::pack_w((int)a, (int)b)
                                     : vo::pk_absdiff_i16(a, b);
    }
};

// ---- vo_lkmath.h, the composites (the per-case bodies of host_check.cpp's hc_bilinear7_u8 / hc_bilinear7_deriv / hc_diff_dot)
UC_HD void unpack7(const uint32_t *pk, int16_t *v7)
{
    for (int k = 0; k < 7; k++)
        v7[k] = (int16_t)((pk[k / 2] >> (16 * (k & 1))) & 0xffff);
}
// u8 top[8], bot[8], i32 w[4] -> i16 val[7] (val[0] = 0x7fff if the unused eighth slot is not zero)
template <bool TWO_STEP>
struct Bilinear {
    static constexpr int IN = 32, OUT = 14;
    static constexpr const char *name() { return TWO_STEP ? "lk_blend7" : "lk_bilinear7_u8"; }
    static UC_HD void run(const void *in, void *out)
    {
        const uint32_t *p = (const uint32_t *)in;
        const int *w = (const int *)in + 4;
        const uint32_t wt = vo::pack_w(w[0], w[1]), wb = vo::pack_w(w[2], w[3]);
        uint32_t o[4];
        if (TWO_STEP) {
            uint32_t pt[7], pb[7];
            vo::lift7(p[0], p[1], pt);
            vo::lift7(p[2], p[3], pb);
            vo::blend7(pt, pb, wt, wb, o);
        } else {
            vo::bilinear7_u8(p[0], p[1], p[2], p[3], wt, wb, o);
        }
        int16_t v[7];
        unpack7(o, v);
        if ((o[3] >> 16) != 0)
            v[0] = 0x7fff;
        for (int k = 0; k < 7; k++)
            ((int16_t *)out)[k] = v[k];
    }
};
// u32 dt[8], db[8] (4 Ix | 4 Iy << 16), i32 w[4] -> i16 ix[7], iy[7] (ix[0] = 0x7fff if an unused slot is not zero)
struct Deriv {
    static constexpr int IN = 80, OUT = 28;
    static constexpr const char *name() { return "lk_bilinear7_deriv"; }
    static UC_HD void run(const void *in, void *out)
    {
        const uint32_t *p = (const uint32_t *)in;
        const int *w = (const int *)in + 16;
        uint32_t dt[8], db[8], ix[4], iy[4];
        for (int k = 0; k < 8; k++) {
            dt[k] = p[k];
            db[k] = p[8 + k];
        }
        vo::bilinear7_deriv(dt, db, vo::pack_w(w[0], w[1]), vo::pack_w(w[2], w[3]), ix, iy);
        int16_t v[14];
        unpack7(ix, v);
        unpack7(iy, v + 7);
        if ((ix[3] >> 16) != 0 || (iy[3] >> 16) != 0)
            v[0] = 0x7fff;
        for (int k = 0; k < 14; k++)
            ((int16_t *)out)[k] = v[k];
    }
};
// i16 val[7], I[7], ix[7] -> i32 sum (val - I) * ix over packed pairs, as the kernel's inner loop
struct DiffDot {
    static constexpr int IN = 42, OUT = 4;
    static constexpr const char *name() { return "lk_diff_dot"; }
    static UC_HD void run(const void *in, void *out)
    {
        const int16_t *a = (const int16_t *)in;
        int acc = 0;
        for (int m = 0; m < 4; m++) {
            uint32_t pk[3];
            for (int j = 0; j < 3; j++) {
                const uint32_t lo = (uint16_t)a[7 * j + 2 * m], hi = 2 * m + 1 < 7 ? (uint16_t)a[7 * j + 2 * m + 1] : 0u;
                pk[j] = lo | (hi << 16);
            }
            acc = vo::sdot2(vo::pk_sub_i16(pk[0], pk[1]), pk[2], acc);
        }
        *(int32_t *)out = acc;
    }
};
// i32 p00, p01, p02, p10, p12, p20, p21, p22 -> u32 (4 Ix | 4 Iy << 16)
struct Scharr {
    static constexpr int IN = 32, OUT = 4;
    static constexpr const char *name() { return "lk_scharr4"; }
    static UC_HD void run(const void *in, void *out)
    {
        const int *p = (const int *)in;
        *(uint32_t *)out = vo::scharr4_packed(p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7]);
    }
};

template <class... Ops>
struct OpList {
};
using AllOps = OpList<Math<0>, Math<1>, Math<2>, Math<3>, Math<4>, Epnp5, P3p4, P3pDeg4, RodV2m, RodM2v, Triangulate, FivePoint, Sampson,
                      Decompose, Cheirality, Solve6, Svd12, LkRaw<0>, LkRaw<1>, LkRaw<2>, LkRaw<3>, LkRaw<4>, LkRaw<5>, LkRaw<6>, LkRaw<7>,
                      LkRaw<8>, LkRaw<9>, LkRaw<10>, LkRaw<11>, LkRaw<12>, LkRaw<13>, Bilinear<false>, Bilinear<true>, Deriv, DiffDot, Scharr>;

} // namespace uc
