/* lk_flags_ref.c -- TEST ONLY.  The expected side of the flags tests (include/vo_flow_flags.h): the checker's own LK arithmetic
 * (oracle/orc_lk.c, included as it is -- every line of lk_level stays the checker's) driven so that it starts at a guess.
 * The checker has flags == 0 wired in: at level == maxLevel it starts at prevPts, at every other level at nextPts * 2.  The driver
 * below is the level loop of orc_calc_optical_flow_pyr_lk with two differences: the guesses are scaled by 2^-(maxLevel + 1) before
 * the loop, and lk_level is told that the deepest level is maxLevel + 1 -- so the top level takes the `nextPts * 2` branch, which
 * is exactly guess * 2^-maxLevel, OpenCV's OPTFLOW_USE_INITIAL_FLOW start.  err == NULL gives the status of a call without an err
 * vector (lk_level makes the final in-bounds check only with one), which is the status of OPTFLOW_LK_GET_MIN_EIGENVALS.
 * Built into its own shared library with the flags of oracle/Makefile (tests/flow_flags_cases.py). */
#include "../../oracle/orc_lk.c"

/* next_pts: the n guesses in, the n results out.  Returns the deepest level tracked on, -1 for bad arguments. */
int lkf_initial_flow(const uint8_t *prev, const uint8_t *next, int w, int h, const float *prev_pts, int n, float *next_pts, uint8_t *status,
                     float *err, int win, int max_level, int max_count, double eps, double min_eig_threshold, int accum_mode, int nthreads)
{
    if (win < 3 || win > 32 || max_level < 0 || max_level > 15)
        return -1;
    if (n == 0)
        return 0;
#ifdef _OPENMP
    if (nthreads <= 0)
        nthreads = omp_get_max_threads();
#else
    nthreads = 1;
#endif
    if (max_count < 0)
        max_count = 0;
    if (max_count > 100)
        max_count = 100;
    if (eps < 0.)
        eps = 0.;
    if (eps > 10.)
        eps = 10.;
    double epsilon = eps * eps;

    OrcLevel pI[16], pJ[16];
    int lI = build_pyramid(prev, w, h, win, max_level, pI);
    int lJ = build_pyramid(next, w, h, win, max_level, pJ);
    int maxLevel = lI < lJ ? lI : lJ;

    for (int i = 0; i < n; i++)
        status[i] = 1;
    if (err)
        for (int i = 0; i < n; i++)
            err[i] = 0;
    for (int i = 0; i < 2 * n; i++) /* difference 1 */
        next_pts[i] *= (float)(1. / (1 << (maxLevel + 1)));

    for (int level = maxLevel; level >= 0; level--) {
        const OrcLevel *I = &pI[level];
        int16_t *d = (int16_t *)malloc(sizeof(int16_t) * 2 * (size_t)I->w * I->h);
        uint8_t *plain = (uint8_t *)malloc((size_t)I->w * I->h);
        for (int y = 0; y < I->h; y++)
            memcpy(plain + (size_t)y * I->w, I->img + (ptrdiff_t)y * I->stride, (size_t)I->w);
        orc_scharr(plain, I->w, I->h, d);
        free(plain);
        size_t dstride = (size_t)(I->w + 2 * win) * 2;
        int16_t *dpad = (int16_t *)calloc(dstride * (I->h + 2 * win), sizeof(int16_t));
        for (int y = 0; y < I->h; y++)
            memcpy(dpad + (size_t)(y + win) * dstride + win * 2, d + (size_t)y * I->w * 2, sizeof(int16_t) * 2 * (size_t)I->w);
        free(d);
        lk_level(I, &pJ[level], dpad, prev_pts, next_pts, status, err, n, win, level, maxLevel + 1 /* difference 2 */, max_count, epsilon,
                 (float)min_eig_threshold, accum_mode, nthreads);
        free(dpad);
    }
    for (int l = 0; l <= lI; l++)
        free(pI[l].buf);
    for (int l = 0; l <= lJ; l++)
        free(pJ[l].buf);
    return maxLevel;
}
