// lk_fit_host.cpp -- TEST ONLY.  A g++ program (its own main; may be built with -fsanitize=address,undefined) over
//   (a) the 32-bit wave sums of vo_dev.h -- wave_sum2_fit_f32 and wave_sum2_f32, the text the CPU emulator runs -- on the vectors of
//       lk_fit_cases.h: each equals (float)(int64 sum) bit for bit, and equals wave_sum2_exact_f32 wherever that one applies;
//   (b) lk_sums_fit (vo_lkmath.h), the level's word that the iteration's sums fit 32 bits, as a proof: over random and adversarial
//       W x W templates (W = 5, 13, 21) of int16 Ixp, Iyp within +-4080, wherever it says yes the exact integers 8160 * sum |Ixp|
//       and 8160 * sum |Iyp| -- what |b1|, |b2| can reach against ANY search image -- are below 2^31.  The structure-tensor sums go
//       in as the kernel has them: the exact integer rounded once to f32.
//     lk_fit_host [out]   prints "OK <vectors> <vectors with a wrapping partial sum> <templates> <yes> <no>", exit 0; else the first
//                         failure, exit 1.  out: the FitOut records, for tests/test_gpu_lk_fit_sums.py to compare the device's with.
#include "hip_emu.h"

#include "../../visual_odom_amd/csrc/vo_dev.h"
#include "../../visual_odom_amd/csrc/vo_lkmath.h"

#include "lk_fit_cases.h"

#include <stdio.h>

static uint32_t bits(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

static int sums(const char *out_file, int &n_cases, int &n_wrap)
{
    const std::vector<FitCase> cases = fit_cases();
    std::vector<FitOut> got(cases.size());
    n_cases = (int)cases.size();
    n_wrap = 0;
    int n_both = 0;
    for (size_t i = 0; i < cases.size(); i++) {
        const FitCase &c = cases[i];
        float r[8] = {};
        emu::run_block(64, 0, 0, 0, [&] {
            const int l = threadIdx.x;
            float f0, f1, e0 = 0.f, e1 = 0.f, g0, g1, h0 = 0.f, h1 = 0.f;
            vo::wave_sum2_fit_f32(c.a[l], c.b[l], f0, f1);
            vo::wave_sum2_f32(c.a[l], c.b[l], true, g0, g1);
            if (c.exact_ok) { // (the same in every lane)
                vo::wave_sum2_exact_f32(c.a[l], c.b[l], e0, e1);
                vo::wave_sum2_f32(c.a[l], c.b[l], false, h0, h1);
            }
            if (l == 0)
                r[0] = f0, r[1] = f1, r[2] = e0, r[3] = e1, r[4] = g0, r[5] = g1, r[6] = h0, r[7] = h1;
        });
        const uint32_t wa = fit_want_bits(c.a), wb = fit_want_bits(c.b);
        const int64_t ta = fit_total(c.a), tb = fit_total(c.b);
        if (ta > INT32_MAX || ta < -(int64_t)INT32_MAX || tb > INT32_MAX || tb < -(int64_t)INT32_MAX) {
            printf("vector %zu: a total outside +-(2^31 - 1): %lld %lld (the generator's fault)\n", i, (long long)ta, (long long)tb);
            return 1;
        }
        bool ok = bits(r[0]) == wa && bits(r[1]) == wb && bits(r[4]) == wa && bits(r[5]) == wb;
        if (c.exact_ok)
            ok = ok && bits(r[2]) == wa && bits(r[3]) == wb && bits(r[6]) == wa && bits(r[7]) == wb;
        if (!ok) {
            printf("vector %zu (exact_ok %d, wraps %d): totals %lld %lld want %08x %08x, fit %08x %08x, exact %08x %08x, sum2(true) %08x %08x, "
                   "sum2(false) %08x %08x\n", i, c.exact_ok, c.wraps, (long long)ta, (long long)tb, wa, wb, bits(r[0]), bits(r[1]), bits(r[2]),
                   bits(r[3]), bits(r[4]), bits(r[5]), bits(r[6]), bits(r[7]));
            return 1;
        }
        got[i] = FitOut{{bits(r[0]), bits(r[1]), c.exact_ok ? bits(r[2]) : 0u, c.exact_ok ? bits(r[3]) : 0u, bits(r[4]), bits(r[5])}};
        n_wrap += c.wraps;
        n_both += c.exact_ok;
    }
    if (n_wrap < 400 || n_both < 400) {
        printf("the list holds %d vectors with a wrapping partial sum and %d where both trees apply: fewer than meant\n", n_wrap, n_both);
        return 1;
    }
    if (out_file) {
        FILE *f = fopen(out_file, "wb");
        if (!f || fwrite(got.data(), sizeof(FitOut), got.size(), f) != got.size() || fclose(f) != 0)
            return 2;
    }
    return 0;
}

// ---- (b) ----------------------------------------------------------------------------------------------------------------------
struct Template {
    int n;
    int16_t ix[441], iy[441];
};
static int n_yes, n_no;
static int check(const Template &t, const char *what)
{
    int64_t a11 = 0, a22 = 0, sx = 0, sy = 0;
    for (int i = 0; i < t.n; i++) {
        if (t.ix[i] > 4080 || t.ix[i] < -4080 || t.iy[i] > 4080 || t.iy[i] < -4080) {
            printf("%s: a sample outside +-4080 (the generator's fault)\n", what);
            return 1;
        }
        a11 += (int64_t)t.ix[i] * t.ix[i];
        a22 += (int64_t)t.iy[i] * t.iy[i];
        sx += t.ix[i] < 0 ? -t.ix[i] : t.ix[i];
        sy += t.iy[i] < 0 ? -t.iy[i] : t.iy[i];
    }
    const bool yes = vo::lk_sums_fit((float)a11, (float)a22);
    (yes ? n_yes : n_no)++;
    // (8192 for 8160: the bound the comment in vo_lkmath.h derives the threshold from)
    if (yes && !(8160 * sx < (1ll << 31) && 8160 * sy < (1ll << 31) && 8192 * sx < (1ll << 31) && 8192 * sy < (1ll << 31))) {
        printf("%s (%d pixels): lk_sums_fit(%lld, %lld) says yes, 8160 * sum |Ixp| = %lld, 8160 * sum |Iyp| = %lld, 2^31 = %lld\n", what, t.n,
               (long long)a11, (long long)a22, (long long)(8160 * sx), (long long)(8160 * sy), 1ll << 31);
        return 1;
    }
    return 0;
}
// v[0 .. n): sum of squares exactly `target`: n - 8 values of one magnitude (random signs), the rest by greedy square roots
static bool squares(FitRng &r, int n, int64_t target, int16_t *v)
{
    int64_t c = (int64_t)sqrt((double)target / (n - 8));
    c = c > 4080 ? 4080 : c;
    int64_t rest = target - (n - 8) * c * c;
    for (int i = 0; i < n - 8; i++)
        v[i] = (int16_t)((r.next() & 1) ? c : -c);
    for (int i = n - 8; i < n; i++) {
        int64_t s = (int64_t)sqrt((double)rest);
        while (s * s > rest)
            s--;
        s = s > 4080 ? 4080 : s;
        v[i] = (int16_t)((r.next() & 1) ? s : -s);
        rest -= s * s;
    }
    return rest == 0;
}
static int predicate(int &n_templates)
{
    if (bits(vo::LK_FIT_RAW_MAX) != vo::LK_FIT_RAW_MAX_BITS || vo::LK_FIT_RAW_MAX != 150000000.f) {
        printf("LK_FIT_RAW_MAX_BITS is not the bit pattern of LK_FIT_RAW_MAX = 1.5e8f\n");
        return 1;
    }
    FitRng r;
    Template t;
    const int wins[3] = {5, 13, 21};
    n_yes = n_no = 0;
    for (int wi = 0; wi < 3; wi++) {
        t.n = wins[wi] * wins[wi];
        // constant +-4080 (the largest sums there are), constant small, a single spike, one axis only
        for (int k = 0; k < 8; k++) {
            const int16_t cx = (int16_t)((k & 1) ? 4080 : -4080), cy = (int16_t)((k & 2) ? 4080 : (k & 4) ? -4080 : 0);
            for (int i = 0; i < t.n; i++)
                t.ix[i] = cx, t.iy[i] = cy;
            if (check(t, "constant +-4080"))
                return 1;
            for (int i = 0; i < t.n; i++)
                t.ix[i] = (int16_t)(cx / 16), t.iy[i] = (int16_t)(cy / 16);
            if (check(t, "constant +-255"))
                return 1;
            memset(t.ix, 0, sizeof(t.ix));
            memset(t.iy, 0, sizeof(t.iy));
            t.ix[(k * 53) % t.n] = cx;
            t.iy[(k * 31) % t.n] = cy;
            if (check(t, "single spike"))
                return 1;
        }
        // one magnitude, random signs (Cauchy-Schwarz holds with equality: the tightest template of its A11raw), some pixels zero
        for (int k = 0; k < 3000; k++) {
            const double lx = log(60.0) + (log(4080.0) - log(60.0)) * (r.next() % 10001) / 10000.0;
            const double ly = log(60.0) + (log(4080.0) - log(60.0)) * (r.next() % 10001) / 10000.0;
            const int16_t cx = (int16_t)exp(lx), cy = (int16_t)exp((k & 3) ? ly : lx * 0.5);
            const uint32_t zero_every = (k % 5 == 0) ? 2 + r.next() % 6 : 0;
            for (int i = 0; i < t.n; i++) {
                const bool z = zero_every && r.next() % zero_every == 0;
                t.ix[i] = z ? 0 : (int16_t)((r.next() & 1) ? cx : -cx);
                t.iy[i] = z ? 0 : (int16_t)((r.next() & 1) ? cy : -cy);
            }
            if (check(t, "one magnitude, random signs"))
                return 1;
        }
        // uniform within an amplitude
        for (int k = 0; k < 3000; k++) {
            const int ax = 1 + (int)(r.next() % 4080), ay = (k & 1) ? 1 + (int)(r.next() % 4080) : ax;
            for (int i = 0; i < t.n; i++)
                t.ix[i] = (int16_t)r.range(-ax, ax), t.iy[i] = (int16_t)r.range(-ay, ay);
            if (check(t, "uniform"))
                return 1;
        }
        // A11raw (or A22raw) an exact integer at the threshold, one f32 ulp (16) and less to either side of it; the other sum small
        // or at the threshold too.  150000000 - 1 ... - 8 round up to the threshold: "no".
        const int off[] = {-48, -32, -17, -16, -9, -8, -7, -1, 0, 1, 7, 8, 9, 16, 17, 32, 48};
        for (int k = 0; k < 17 * 3 * 20; k++) {
            const int64_t target = 150000000ll + off[k % 17];
            const int mode = (k / 17) % 3;
            memset(t.ix, 0, sizeof(t.ix));
            memset(t.iy, 0, sizeof(t.iy));
            if (!squares(r, t.n, target, mode == 1 ? t.iy : t.ix) || (mode == 2 && !squares(r, t.n, 150000000ll - 16, t.iy))) {
                printf("no template with a sum of squares of %lld (the generator's fault)\n", (long long)target);
                return 1;
            }
            if (check(t, "at the threshold"))
                return 1;
        }
    }
    n_templates = n_yes + n_no;
    if (4 * n_yes < n_templates || 4 * n_no < n_templates) {
        printf("%d templates: %d yes, %d no -- less than a quarter on one side\n", n_templates, n_yes, n_no);
        return 1;
    }
    return 0;
}

int main(int argc, char **argv)
{
    int n_cases = 0, n_wrap = 0, n_templates = 0;
    int rc = sums(argc > 1 ? argv[1] : nullptr, n_cases, n_wrap);
    if (rc == 0)
        rc = predicate(n_templates);
    if (rc)
        return rc;
    printf("OK %d %d %d %d %d\n", n_cases, n_wrap, n_templates, n_yes, n_no);
    return 0;
}
