// lk_fit_cases.h -- TEST ONLY.  The per-lane vectors of the 32-bit wave sums (vo_dev.h: wave_sum2_fit_f32, wave_sum2_f32), shared by
// the g++ program over the emulator text (lk_fit_host.cpp) and the program that runs the instructions on gfx950 (lk_fit_check.hip).
// A case is 64 lane values for each of the two sums.  wave_sum2_fit_f32's precondition is on the TOTALS only (|total| < 2^31, the
// lanes arbitrary int32, partial sums free to wrap), and the list is built around that:
//   * random lanes below 2^24, below 2^28 (wave_sum2_exact_f32's precondition holds too: the two functions must agree);
//   * 31 pairs (x, -x) with |x| up to 2^31 - 1 at shuffled lanes plus two lanes that hold the wanted total: whichever way the tree
//     pairs them, most partial sums leave 32 bits, several times over, and the total is the one chosen;
//   * whole rows of +2^30 against whole rows of -2^30 (every partial sum of the first four steps wraps), total chosen likewise;
//   * chosen totals: +-(2^31 - 1), 0, +-2^24 +- 1 (where rounding to f32 begins), +-(2^31 - 65) (rounds to 2^31 - 128, not 2^31),
//     random ones -- and each of them in one sum with the other sum small.
// Want: (float)(int64 sum of the lanes), bit for bit.
#pragma once

#include <stdint.h>
#include <string.h>

#include <vector>

struct FitCase {
    int32_t a[64], b[64];
    int32_t exact_ok; // every |lane| < 2^28: wave_sum2_exact_f32 applies as well
    int32_t wraps;    // a partial sum of the tree leaves 32 bits in at least one of the two sums
};
struct FitOut { // bit patterns: fit a, fit b, exact a, exact b (0 where it does not apply), wave_sum2_f32(fit = true) a, b
    uint32_t v[6];
};

struct FitRng {
    uint64_t s = 88172645463325252ull;
    uint32_t next()
    {
        s ^= s << 13;
        s ^= s >> 7;
        s ^= s << 17;
        return (uint32_t)(s >> 16);
    }
    int32_t range(int64_t lo, int64_t hi) { return (int32_t)(lo + (int64_t)((((uint64_t)next() << 32) | next()) % (uint64_t)(hi - lo + 1))); }
};

inline int64_t fit_total(const int32_t v[64])
{
    int64_t s = 0;
    for (int l = 0; l < 64; l++)
        s += v[l];
    return s;
}
inline uint32_t fit_want_bits(const int32_t v[64])
{
    const float f = (float)fit_total(v);
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}
// does a partial sum of wave_sum2_fit_f32's tree over v leave int32?  (the tree: l + (l + 32), then xor 1, 2, rows, the two rows)
inline bool fit_tree_wraps(const int32_t v[64])
{
    int64_t t[32];
    bool w = false;
    for (int l = 0; l < 32; l++)
        t[l] = (int64_t)v[l] + v[l + 32];
    for (int n = 32; n >= 1; n /= 2) { // (any binary tree over the 32 pair sums shows the same: magnitudes, not the exact shape, matter)
        for (int l = 0; l < n; l++)
            w = w || t[l] > INT32_MAX || t[l] < INT32_MIN;
        for (int l = 0; l < n / 2; l++)
            t[l] = t[2 * l] + t[2 * l + 1];
    }
    return w;
}

// 64 lanes of cancelling pairs at shuffled positions and two lanes that hold `total` (|total| < 2^31)
inline void fit_pairs(FitRng &r, int64_t total, int32_t v[64])
{
    int pos[64];
    for (int l = 0; l < 64; l++)
        pos[l] = l;
    for (int l = 63; l > 0; l--) {
        const int k = (int)(r.next() % (uint32_t)(l + 1)), t = pos[l];
        pos[l] = pos[k];
        pos[k] = t;
    }
    for (int p = 0; p < 31; p++) {
        const int32_t x = r.range(-(int64_t)INT32_MAX, INT32_MAX);
        v[pos[2 * p]] = x;
        v[pos[2 * p + 1]] = -x;
    }
    const int64_t h = total / 2;
    v[pos[62]] = (int32_t)h;
    v[pos[63]] = (int32_t)(total - h);
}
// rows 0 and 2 (lanes 0-15, 32-47) at +2^30, rows 1 and 3 at -2^30, `total` added in lanes 20 and 52
inline void fit_rows(int64_t total, int32_t v[64])
{
    for (int l = 0; l < 64; l++)
        v[l] = ((l >> 4) & 1) ? -(1 << 30) : (1 << 30);
    const int64_t h = total / 2;
    // the total goes into two lanes of the NEGATIVE rows (room for any total below 2^31: -2^30 + total / 2 stays inside int32)
    v[20] = (int32_t)(-(int64_t)(1 << 30) + h);
    v[52] = (int32_t)(-(int64_t)(1 << 30) + (total - h));
}
inline void fit_random(FitRng &r, int32_t bound, int32_t v[64])
{
    for (int l = 0; l < 64; l++)
        v[l] = r.range(-(int64_t)bound, bound);
}

inline std::vector<FitCase> fit_cases()
{
    std::vector<FitCase> out;
    FitRng r;
    const int64_t M = INT32_MAX; // 2^31 - 1
    const int64_t chosen[] = {M, -M, 0, (1 << 24) + 1, (1 << 24) - 1, -(1 << 24) + 1, -(1 << 24) - 1, M - 64, -(M - 64), (1ll << 30) + 1, 1, -1};
    auto push = [&](FitCase &c) {
        c.exact_ok = 1;
        for (int l = 0; l < 64; l++)
            if (c.a[l] >= (1 << 28) || c.a[l] <= -(1 << 28) || c.b[l] >= (1 << 28) || c.b[l] <= -(1 << 28))
                c.exact_ok = 0;
        c.wraps = fit_tree_wraps(c.a) || fit_tree_wraps(c.b);
        out.push_back(c);
    };
    FitCase c;
    for (int k = 0; k < 256; k++) { // random lanes, both preconditions hold (64 * 2^24 = 2^30; 64 lanes below 2^28 may exceed: kept below 2^31 by the draw)
        fit_random(r, (1 << 24) - 1, c.a);
        fit_random(r, k & 1 ? (1 << 24) - 1 : 1000, c.b);
        push(c);
    }
    for (int k = 0; k < 256; k++) { // lanes up to 2^28 - 1 in cancelling pairs: the exact tree's precondition at its limit, totals chosen
        const int64_t ta = k < 12 ? chosen[k] : r.range(-M, M), tb = r.range(-M, M);
        for (int s = 0; s < 2; s++) {
            int32_t *v = s ? c.b : c.a;
            const int64_t t = s ? tb : ta;
            for (int l = 0; l < 32; l++) {
                const int32_t x = r.range(-((1 << 28) - 1), (1 << 28) - 1);
                v[2 * l] = x;
                v[2 * l + 1] = -x;
            }
            for (int l = 0; l < 16; l++) // the total over 16 lanes: each share below 2^27, the lane stays below 2^28 ...
                v[4 * l] = (int32_t)(t / 16 + (l == 0 ? t % 16 : 0)), v[4 * l + 1] = 0; // ... its partner gives up its value
        }
        push(c);
    }
    for (int k = 0; k < 512; k++) { // arbitrary lanes, wrapping partial sums, totals chosen or random; one sum at the limit with the other small
        const int64_t ta = k < 12 ? chosen[k] : r.range(-M, M);
        const int64_t tb = (k % 3 == 0) ? r.range(-1000, 1000) : (k % 3 == 1) ? chosen[(k / 3) % 12] : r.range(-M, M);
        if (k & 1) {
            fit_pairs(r, ta, c.a);
            fit_pairs(r, tb, c.b);
        } else {
            fit_pairs(r, tb, c.a);
            fit_pairs(r, ta, c.b);
        }
        push(c);
    }
    for (int k = 0; k < 12; k++) { // whole rows against whole rows
        fit_rows(chosen[k], c.a);
        fit_rows(chosen[11 - k], c.b);
        push(c);
        fit_rows(chosen[k], c.a);
        fit_random(r, 100, c.b);
        push(c);
    }
    return out;
}
