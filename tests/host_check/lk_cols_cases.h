// lk_cols_cases.h -- TEST ONLY.  The unit vectors of the vertical-pair samplers of vo_lkmath.h (lift8_cols + blend7_cols,
// bilinear7_deriv_cols) and the two ways to evaluate a case: through the new composites and through the horizontal-pair ones
// they must equal (bilinear7_u8, bilinear7_deriv).  Shared by lk_cols_host.cpp (g++: the host text of the wrappers) and
// lk_cols_check.hip (the same vectors through the instructions on gfx950).
//
// A case = one weight pair (a, b) x one pattern.  The weights are formed as lk.hip forms them (f32 products of (1 - a) 2^14,
// a 2^14, 1 - b, b, rounded half to even; iw11 = 2^14 - the other three).  (a, b) run over a grid G x G, G = 32 coarse steps of
// 1/32, 8 steps of 2^-12 from 0 and below 1, 0.5 + 1/64, 1 - 2^-20, and twenty values k 2^-14 that pair up to k k' = 8190 .. 8192:
// there a b 2^14 is just below 1/2 while the other three products round up, so they add up to 2^14 + 1 and iw11 = -1 (at least
// ten pairs and their mirror images; the programs count the cases and refuse a grid without any).  Patterns: pixel bytes all 0,
// all 255, alternating 0 / 255 in both phases with the lower row equal or inverted, the rows 0 over 255 and 255 over 0, and two
// random ones; Scharr samples (stored x 4, both halves of the dword) all +16320, all -16320, alternating in sign by column, by
// row and by both, x against y, and two random ones.
#pragma once

#include "../../visual_odom_amd/csrc/vo_lkmath.h"

#include <math.h>
#include <vector>

struct ColsCase {
    uint32_t pix[4];       // t_lo, t_hi, b_lo, b_hi: 8 bytes of the upper row, 8 of the lower
    uint32_t dt[8], db[8]; // (4 Ix | 4 Iy << 16) of the 8 columns, upper / lower row
    int32_t w[4];          // iw00, iw01, iw10, iw11
};
struct ColsOut {
    uint32_t val[4], ix[4], iy[4]; // packed int16 pairs, as the composites return them
};

VO_HD void cols_new(const ColsCase &c, ColsOut &o)
{
    const uint32_t wl = vo::pack_w(c.w[0], c.w[2]), wr = vo::pack_w(c.w[1], c.w[3]);
    uint32_t col[8];
    vo::lift8_cols(c.pix[0], c.pix[1], c.pix[2], c.pix[3], col);
    vo::blend7_cols(col, wl, wr, o.val);
    vo::bilinear7_deriv_cols(c.dt, c.db, wl, wr, o.ix, o.iy);
}

VO_HD void cols_old(const ColsCase &c, ColsOut &o)
{
    const uint32_t wt = vo::pack_w(c.w[0], c.w[1]), wb = vo::pack_w(c.w[2], c.w[3]);
    vo::bilinear7_u8(c.pix[0], c.pix[1], c.pix[2], c.pix[3], wt, wb, o.val);
    vo::bilinear7_deriv(c.dt, c.db, wt, wb, o.ix, o.iy);
}

static inline bool cols_same(const ColsOut &a, const ColsOut &b)
{
    for (int m = 0; m < 4; m++)
        if (a.val[m] != b.val[m] || a.ix[m] != b.ix[m] || a.iy[m] != b.iy[m])
            return false;
    return true;
}

static inline std::vector<float> cols_grid()
{
    std::vector<float> g;
    for (int k = 0; k < 32; k++)
        g.push_back((float)k / 32.f);
    for (int k = 1; k <= 8; k++)
        g.push_back((float)k / 4096.f), g.push_back(1.f - (float)k / 4096.f);
    for (int k : {18, 455, 21, 390, 23, 356, 24, 341, 26, 315, 30, 273, 31, 264, 33, 248, 35, 234, 39, 210})
        g.push_back((float)k / 16384.f);
    g.push_back(0.5f + 1.f / 64.f);
    g.push_back(1.f - 1.f / 1048576.f);
    return g;
}

constexpr int COLS_PATTERNS = 8;

// every case, and the number of them with iw11 < 0
static inline std::vector<ColsCase> cols_cases(int *n_negative)
{
    const std::vector<float> g = cols_grid();
    std::vector<ColsCase> out;
    out.reserve(g.size() * g.size() * COLS_PATTERNS);
    uint64_t s = 0x9e3779b97f4a7c15ull; // xorshift64*
    auto rnd = [&s]() {
        s ^= s >> 12, s ^= s << 25, s ^= s >> 27;
        return (uint32_t)((s * 0x2545f4914f6cdd1dull) >> 32);
    };
    auto sample = [](int x, int y) { return ((uint32_t)x & 0xffffu) | ((uint32_t)y << 16); };
    auto random_sample = [&]() { // (one draw per statement: the order of evaluation of call arguments is the compiler's choice)
        const int x = 4 * ((int)(rnd() % 8161u) - 4080);
        const int y = 4 * ((int)(rnd() % 8161u) - 4080);
        return sample(x, y);
    };
    *n_negative = 0;
    for (float a : g)
        for (float b : g) {
            const float sc = 16384.f, a1 = (1.f - a) * sc, a0 = a * sc, b1 = 1.f - b;
            const int w00 = (int)lrintf(a1 * b1), w01 = (int)lrintf(a0 * b1), w10 = (int)lrintf(a1 * b), w11 = 16384 - w00 - w01 - w10;
            for (int p = 0; p < COLS_PATTERNS; p++) {
                ColsCase c;
                c.w[0] = w00, c.w[1] = w01, c.w[2] = w10, c.w[3] = w11;
                const uint32_t alt = 0xff00ff00u; // bytes 0, 255, 0, 255
                const uint32_t pix[COLS_PATTERNS][4] = {{0, 0, 0, 0}, {~0u, ~0u, ~0u, ~0u}, {alt, alt, alt, alt}, {~alt, ~alt, ~alt, ~alt},
                                                        {alt, alt, ~alt, ~alt}, {0, 0, ~0u, ~0u}, {rnd(), rnd(), rnd(), rnd()},
                                                        {rnd(), rnd(), rnd(), rnd()}};
                for (int k = 0; k < 4; k++)
                    c.pix[k] = p == 5 && ((out.size() / COLS_PATTERNS) & 1) ? ~pix[p][k] : pix[p][k]; // 0 over 255, 255 over 0
                const int M = 16320;
                for (int k = 0; k < 8; k++) {
                    const int sk = k & 1 ? -M : M;
                    switch (p) {
                    case 0: c.dt[k] = c.db[k] = sample(M, M); break;
                    case 1: c.dt[k] = c.db[k] = sample(-M, -M); break;
                    case 2: c.dt[k] = c.db[k] = sample(sk, sk); break;
                    case 3: c.dt[k] = sample(M, M), c.db[k] = sample(-M, -M); break;
                    case 4: c.dt[k] = sample(sk, -sk), c.db[k] = sample(-sk, sk); break;
                    case 5: c.dt[k] = c.db[k] = sample(M, -M); break;
                    default: // true Scharr samples are in [-4080, 4080], stored x 4
                        c.dt[k] = random_sample();
                        c.db[k] = random_sample();
                    }
                }
                out.push_back(c);
            }
            *n_negative += w11 < 0 ? COLS_PATTERNS : 0;
        }
    return out;
}

// the plain restatement, int64: DESCALE(t[k] iw00 + t[k+1] iw01 + b[k] iw10 + b[k+1] iw11, n), n = 9 for pixels (the template's
// I * 32), 14 for Scharr samples stored x 4 (the true derivative)
static inline void cols_plain(const ColsCase &c, ColsOut &o)
{
    auto byte = [&c](int row, int k) { return (int64_t)((c.pix[2 * row + k / 4] >> (8 * (k % 4))) & 0xff); };
    auto half = [](uint32_t d, int hi) { return (int64_t)(int16_t)(hi ? d >> 16 : d & 0xffff); };
    int64_t v[8] = {0}, x[8] = {0}, y[8] = {0};
    for (int k = 0; k < 7; k++) {
        v[k] = (byte(0, k) * c.w[0] + byte(0, k + 1) * c.w[1] + byte(1, k) * c.w[2] + byte(1, k + 1) * c.w[3] + (1 << 8)) >> 9;
        x[k] = (half(c.dt[k], 0) * c.w[0] + half(c.dt[k + 1], 0) * c.w[1] + half(c.db[k], 0) * c.w[2] + half(c.db[k + 1], 0) * c.w[3] + (1 << 15)) >> 16;
        y[k] = (half(c.dt[k], 1) * c.w[0] + half(c.dt[k + 1], 1) * c.w[1] + half(c.db[k], 1) * c.w[2] + half(c.db[k + 1], 1) * c.w[3] + (1 << 15)) >> 16;
    }
    for (int m = 0; m < 4; m++) {
        o.val[m] = ((uint32_t)v[2 * m] & 0xffffu) | ((uint32_t)v[2 * m + 1] << 16);
        o.ix[m] = ((uint32_t)x[2 * m] & 0xffffu) | ((uint32_t)x[2 * m + 1] << 16);
        o.iy[m] = ((uint32_t)y[2 * m] & 0xffffu) | ((uint32_t)y[2 * m + 1] << 16);
    }
}
