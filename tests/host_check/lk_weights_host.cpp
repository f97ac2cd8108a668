// lk_weights_host.cpp -- TEST ONLY.  A g++ program (its own main; may be built with -fsanitize=address,undefined) over the text of
// vo_lkmath.h that the CPU emulator runs:
//   (a) lk_weights_packed<COLS> -- (a * b1, b * a1) as one pair into the packed scale-and-round, a1 * b1 beside it -- equals, bit for
//       bit and for both packings, the statement it replaced (weights_before below: a1 * b1 paired with a * b1, round 11's text) and
//       the plain restatement (three rounded products, cvRound by nearbyint, the fourth weight by subtraction), over
//         * two dense grids of fraction pairs, k / 256 x k / 256 and (k + 0.37) / 251 x (k + 0.37) / 251;
//         * every pair of the 64 largest and the 64 smallest floats of [0, 1);
//         * a 101 x 101 grid over 3.0e-5 .. 3.25e-5, where iw00 = 16383 and iw01 = iw10 = 1 leave iw11 = -1;
//   (b) blend7_cols with the caller's word on the sign of iw11 equals blend7_cols without it and bilinear7_u8 on the row packing,
//       on random pixel cells under every weight pair of the third set and a sample of the others.
//     lk_weights_host   prints "OK <pairs> <pairs with iw11 = -1> <blends> <blends with iw11 = -1>", exit 0; else the first
//                       failure, exit 1.
#include "../../visual_odom_amd/csrc/vo_lkmath.h"

#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

// round 11's lk_weights_packed, as it stood in lk.hip
template <bool COLS>
static void weights_before(float a, float b, uint32_t &w0, uint32_t &w1)
{
    const float s = (float)(1 << vo::LK_W_BITS), magic = 12582912.f;
    typedef float F32x2 __attribute__((vector_size(8)));
    const F32x2 p = {a, b}, q = 1.f - p, pswap = {b, a};
    const F32x2 x = q * pswap; // (a1 * b, b1 * a)
    const uint32_t r00 = vo::f32_bits(fmaf(q[0] * q[1], s, magic));
    const uint32_t r01 = vo::f32_bits(fmaf(x[1], s, magic));
    const uint32_t r10 = vo::f32_bits(fmaf(x[0], s, magic));
    const uint32_t iw11 = ((1u << vo::LK_W_BITS) + 3u * 0x4B400000u) - (r00 + r01 + r10);
    w0 = vo::perm_b32(COLS ? r10 : r01, r00, vo::VO_SEL_LO16);
    w1 = vo::perm_b32(iw11, COLS ? r01 : r10, vo::VO_SEL_LO16);
}

// OpenCV's statement: cvRound of the three products (round half to even: the default rounding mode), the fourth by subtraction
static void weights_plain(float a, float b, int iw[4])
{
    const volatile float a1 = 1.f - a, b1 = 1.f - b; // (volatile: every product rounded to f32 before the scale)
    const volatile float p00 = a1 * b1, p01 = a * b1, p10 = a1 * b;
    iw[0] = (int)nearbyint((double)p00 * 16384.0);
    iw[1] = (int)nearbyint((double)p01 * 16384.0);
    iw[2] = (int)nearbyint((double)p10 * 16384.0);
    iw[3] = 16384 - iw[0] - iw[1] - iw[2];
}

static uint32_t pack(int lo, int hi)
{
    return (uint32_t)(lo & 0xffff) | ((uint32_t)hi << 16);
}

struct Rng {
    uint64_t s;
    uint32_t next()
    {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(s >> 33);
    }
};

static long long n_pairs, n_neg, n_blends, n_blend_neg;

static bool check_blend(float a, float b, Rng &rng)
{
    uint32_t wl, wr, wt, wb;
    vo::lk_weights_cols(a, b, wl, wr);
    vo::lk_weights(a, b, wt, wb);
    const uint32_t t_lo = rng.next() | (rng.next() << 31), t_hi = rng.next() | (rng.next() << 31);
    uint32_t b_lo = rng.next() | (rng.next() << 31), b_hi = rng.next() | (rng.next() << 31);
    if (rng.next() & 1) // bright lower rows: where a negative weight bites
        b_lo = b_hi = 0xffffffffu;
    uint32_t col[8], with[4], without[4], rows[4];
    vo::lift8_cols(t_lo, t_hi, b_lo, b_hi, col);
    const bool neg = (wr & 0x80000000u) != 0;
    vo::blend7_cols(col, wl, wr, neg, with);
    vo::blend7_cols(col, wl, wr, without);
    vo::bilinear7_u8(t_lo, t_hi, b_lo, b_hi, wt, wb, rows);
    n_blends++;
    n_blend_neg += neg;
    if (memcmp(with, without, 16) != 0 || memcmp(with, rows, 16) != 0) {
        printf("blend (a, b) = (%a, %a), neg %d: with the sign %08x %08x %08x %08x, without %08x %08x %08x %08x, by rows %08x %08x %08x %08x\n", a, b, neg,
               with[0], with[1], with[2], with[3], without[0], without[1], without[2], without[3], rows[0], rows[1], rows[2], rows[3]);
        return false;
    }
    return true;
}

static bool check_pair(float a, float b)
{
    uint32_t n0, n1, o0, o1, r0, r1, q0, q1;
    int iw[4];
    vo::lk_weights_packed<true>(a, b, n0, n1);
    weights_before<true>(a, b, o0, o1);
    vo::lk_weights_packed<false>(a, b, r0, r1);
    weights_before<false>(a, b, q0, q1);
    weights_plain(a, b, iw);
    n_pairs++;
    n_neg += iw[3] < 0;
    const bool ok = n0 == o0 && n1 == o1 && r0 == q0 && r1 == q1 && n0 == pack(iw[0], iw[2]) && n1 == pack(iw[1], iw[3]) && r0 == pack(iw[0], iw[1]) &&
                    r1 == pack(iw[2], iw[3]) && iw[3] >= -1;
    if (!ok)
        printf("(a, b) = (%a, %a): by column %08x %08x, before %08x %08x; by row %08x %08x, before %08x %08x; plain %d %d %d %d\n", a, b, n0, n1, o0, o1,
               r0, r1, q0, q1, iw[0], iw[1], iw[2], iw[3]);
    return ok;
}

int main()
{
    Rng rng = {20261020};
    // two dense grids
    for (int i = 0; i < 256; i++)
        for (int j = 0; j < 256; j++) {
            const float a = (float)i / 256.f, b = (float)j / 256.f;
            if (!check_pair(a, b) || ((i * 256 + j) % 61 == 0 && !check_blend(a, b, rng)))
                return 1;
        }
    for (int i = 0; i < 251; i++)
        for (int j = 0; j < 251; j++) {
            const float a = ((float)i + 0.37f) / 251.f, b = ((float)j + 0.37f) / 251.f;
            if (!check_pair(a, b) || ((i * 251 + j) % 61 == 0 && !check_blend(a, b, rng)))
                return 1;
        }
    // the 64 smallest and the 64 largest floats of [0, 1), every pair
    std::vector<float> ends;
    float v = 0.f;
    for (int i = 0; i < 64; i++, v = nextafterf(v, 1.f))
        ends.push_back(v);
    v = nextafterf(1.f, 0.f);
    for (int i = 0; i < 64; i++, v = nextafterf(v, 0.f))
        ends.push_back(v);
    for (float a : ends)
        for (float b : ends)
            if (!check_pair(a, b) || !check_blend(a, b, rng))
                return 1;
    // around iw11 = -1
    const long long neg_before = n_neg;
    for (int i = 0; i <= 100; i++)
        for (int j = 0; j <= 100; j++) {
            const float a = 3.0e-5f + 2.5e-8f * (float)i, b = 3.0e-5f + 2.5e-8f * (float)j;
            if (!check_pair(a, b) || !check_blend(a, b, rng))
                return 1;
        }
    if (n_neg - neg_before < 100 || n_blend_neg < 100) {
        printf("only %lld pairs and %lld blends with iw11 = -1\n", n_neg - neg_before, n_blend_neg);
        return 1;
    }
    printf("OK %lld %lld %lld %lld\n", n_pairs, n_neg, n_blends, n_blend_neg);
    return 0;
}
