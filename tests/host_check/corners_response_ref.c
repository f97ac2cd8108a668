/* corners_response_ref.c -- TEST ONLY.  cv::cornerMinEigenVal(img, out, B, 3), cv::cornerHarris(img, out, B, 3, k) and
 * cv::goodFeaturesToTrack(img, pts, maxCorners, qualityLevel, minDistance, mask, B, useHarrisDetector, k) of OpenCV 4.5.x for 8-bit
 * input and B = 3 or 5, restated step for step in plain serial C from knowledge of upstream (nothing is linked or copied); each step
 * cites the upstream function it restates.  It is the specification the device path of include/vo_corners_response.h is held to.
 * ARGUED, NOT MEASURED: no OpenCV is linked here; tools/opencv_crosscheck.py pins it on a machine that has one.  Build with
 * -ffp-contract=off: upstream's scalar paths are unfused, and so is this.  At (3, min-eigen) and without a mask it must equal
 * corners_ref.c bit for bit; tests/test_corners_response_ref.py holds it to that.
 *
 * Test-only switches.  `trap`: 1 computes the box sum's border samples from the REFLECTED SOURCE instead of reflecting the cov image
 * (the mistake step 2 warns of; at B = 5 the border is two samples deep).  `order`: 0 = upstream's running column sum (the
 * specification), 1 = a plain B-term sum.  `form`: 0 = calcHarris's scalar text (the specification), 1 = its universal-intrinsics
 * loop, which a real x86 build runs for all but the tail columns: the same expression entirely in f32 with (float)k.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

/* cv::borderInterpolate(p, len, BORDER_REFLECT_101) */
static int refl(int p, int len)
{
    if (len == 1)
        return 0;
    while (p < 0 || p >= len)
        p = p < 0 ? -p : 2 * (len - 1) - p;
    return p;
}

static float pix(const uint8_t *img, int w, int h, int stride, int x, int y) { return (float)img[(size_t)refl(y, h) * stride + refl(x, w)]; }

/* Step 1, cv::Sobel(src, CV_32F, 1, 0, 3, scale) / (0, 1) inside cornerEigenValsVecs (corner.cpp): scale = 1 / (255 * 2^(3-1) *
 * block_size), a double (aperture 3, 8-bit input); cv::Sobel multiplies it into the SMOOTHING kernel (`if (dx == 0) kx *= scale;
 * else ky *= scale`), an f32 Mat scaled by (float)scale, so its taps are sf, 2 sf, sf with sf = (float)(1.0 / 3060.0) at B = 3 and
 * (float)(1.0 / 5100.0) at B = 5.  sepFilter2D 8U -> 32F with a 32F intermediate: rows by RowFilter<uchar, float, RowNoVec> (s = k0
 * p(x-1); s += k1 p(x); s += k2 p(x+1), f32), columns by SymmColumnSmallFilter (symmetric: (S0 + S2) * k1 + S1 * k0; the
 * [-1, 0, 1] kernel: S2 - S0).  The source is read at x, y of the SOURCE image, which may lie outside it (REFLECT_101). */
static void sobel(const uint8_t *img, int w, int h, int stride, int block, int x, int y, float *dx, float *dy)
{
    const float sf = (float)(1.0 / (255.0 * 4.0 * block)), sf2 = sf * 2.f;
    float rd[3], rs[3]; /* rows y - 1, y, y + 1: the [-1, 0, 1] row and the [sf, 2 sf, sf] row */
    for (int j = 0; j < 3; j++) {
        const float a = pix(img, w, h, stride, x - 1, y + j - 1), b = pix(img, w, h, stride, x, y + j - 1), c = pix(img, w, h, stride, x + 1, y + j - 1);
        float s = -1.f * a;
        s += 0.f * b;
        s += 1.f * c;
        rd[j] = s;
        s = sf * a;
        s += sf2 * b;
        s += sf * c;
        rs[j] = s;
    }
    *dx = (rd[0] + rd[2]) * sf + rd[1] * sf2;
    *dy = rs[2] - rs[0];
}

/* Steps 1 - 3: out [h][w], tight.  block 3 or 5; harris 0: calcMinEigenVal, 1: calcHarris with k.  Returns 0, -1 on a bad argument
 * or no memory. */
int crr_map(const uint8_t *img, int w, int h, int stride, int block, int harris, double k, float *out, int trap, int order, int form)
{
    if (!img || !out || w < 1 || h < 1 || stride < w || (block != 3 && block != 5))
        return -1;
    const int R = block / 2;
    const size_t n = (size_t)w * h;
    float *cov = (float *)malloc(sizeof(float) * 3 * n);
    double *rows = (double *)malloc(sizeof(double) * 3 * (size_t)w * (h + 2 * R)); /* row sums of rows -R .. h - 1 + R */
    if (!cov || !rows) {
        free(cov);
        free(rows);
        return -1;
    }
    /* cornerEigenValsVecs: cov = (dx * dx, dx * dy, dy * dy) in f32 */
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            float dx, dy;
            sobel(img, w, h, stride, block, x, y, &dx, &dy);
            float *c = cov + 3 * ((size_t)y * w + x);
            c[0] = dx * dx;
            c[1] = dx * dy;
            c[2] = dy * dy;
        }
    /* Step 2, cv::boxFilter(cov, cov, CV_32F, Size(B, B), Point(-1, -1), false, BORDER_REFLECT_101): sumType CV_64F.
     * THE TRAP: the border samples are the COV image reflected, R positions deep.  They are not cov of the reflected source: there
     * dx(-1) = -dx(1), so dx * dy would change sign on a one-sided border (at a corner both factors flip and the sign is right
     * again).  RowSum<float, double>: the ksize == 3 branch is D[x] = (ST)S[x-1] + (ST)S[x] + (ST)S[x+1] and the ksize == 5 branch
     * D[x] = (ST)S[x-2] + (ST)S[x-1] + (ST)S[x] + (ST)S[x+1] + (ST)S[x+2], both left to right.  (Every other ksize takes the branch
     * with a running sum along the row: not restated, not built.) */
    for (int y = -R; y < h + R; y++)
        for (int x = 0; x < w; x++)
            for (int c = 0; c < 3; c++) {
                double s = 0; /* (never read) */
                for (int i = -R; i <= R; i++) {
                    float v;
                    if (trap && (x + i < 0 || x + i >= w || y < 0 || y >= h)) {
                        float dx, dy;
                        sobel(img, w, h, stride, block, x + i, y, &dx, &dy);
                        v = c == 0 ? dx * dx : c == 1 ? dx * dy : dy * dy;
                    } else
                        v = cov[3 * ((size_t)refl(y, h) * w + refl(x + i, w)) + c];
                    s = i == -R ? (double)v : s + (double)v;
                }
                rows[3 * ((size_t)(y + R) * w + x) + c] = s;
            }
    /* ColumnSum<double, float> (the generic template, at every ksize), one FilterEngine pass over the whole image: SUM = 0, then
     * SUM += row for the first B - 1 rows (-R .. R - 1) in order; then per row y: s0 = SUM + row(y + R); D = (float)s0; SUM = s0 -
     * row(y - R) -- a RUNNING sum down the column.  These f64 operations are not exact in general, and an inexact one leaves a
     * residual in SUM that every row below inherits: the order is part of the result.  order = 1 is the plain sum of the B rows,
     * top to bottom. */
    for (int x = 0; x < w; x++)
        for (int c = 0; c < 3; c++) {
            double sum = 0;
            for (int j = 0; j < block - 1; j++)
                sum += rows[3 * ((size_t)j * w + x) + c];
            for (int y = 0; y < h; y++) {
                const double rp = rows[3 * ((size_t)(y + 2 * R) * w + x) + c], rm = rows[3 * ((size_t)y * w + x) + c];
                double s0;
                if (order == 0) {
                    s0 = sum + rp;
                    sum = s0 - rm;
                } else {
                    s0 = rm;
                    for (int j = 1; j < block; j++)
                        s0 = s0 + rows[3 * ((size_t)(y + j) * w + x) + c];
                }
                cov[3 * ((size_t)y * w + x) + c] = (float)s0; /* (in place: the column below reads `rows`, not cov) */
            }
        }
    /* Step 3 (corner.cpp).  calcMinEigenVal, f32: a = 0.5 cov0, b = cov1, c = 0.5 cov2; (a + c) - sqrt((a - c)(a - c) + b b).
     * calcHarris, the scalar text: dst = (float)(a * c - b * b - k * (a + c) * (a + c)) with float a, b, c (no halving) and double k:
     * a * c, b * b and their difference are f32 operations; k * (a + c) is a double times the f32 sum, promoted; times (a + c) again;
     * the subtraction in f64; one cast.  form = 1 is the vector loop: v_float32 k4 = (float)k; a * c - b * b - k4 * (a + c) * (a + c)
     * with every operation in f32. */
    for (size_t i = 0; i < n; i++) {
        if (harris) {
            const float a = cov[3 * i], b = cov[3 * i + 1], c = cov[3 * i + 2];
            if (form == 0)
                out[i] = (float)(a * c - b * b - k * (a + c) * (a + c));
            else {
                const float kf = (float)k;
                out[i] = (a * c - b * b) - (kf * (a + c)) * (a + c);
            }
        } else {
            const float a = cov[3 * i] * 0.5f, b = cov[3 * i + 1], c = cov[3 * i + 2] * 0.5f;
            out[i] = (a + c) - sqrtf((a - c) * (a - c) + b * b);
        }
    }
    free(cov);
    free(rows);
    return 0;
}

static const float *g_base; /* (qsort has no context argument; serial test code) */
/* greaterThanPtr (featureselect.cpp): value descending, ties by the HIGHER address first */
static int by_quality(const void *pa, const void *pb)
{
    const int a = *(const int *)pa, b = *(const int *)pb;
    if (g_base[a] > g_base[b])
        return -1;
    if (g_base[a] < g_base[b])
        return 1;
    return a > b ? -1 : a < b ? 1 : 0;
}

/* Steps 4 - 7, cv::goodFeaturesToTrack (featureselect.cpp) on the map of crr_map(form 0, order 0).  mask: h rows of w bytes,
 * mask_stride apart, non-zero = allowed, or NULL.  pts [cap][2] takes the first cap corners as Point2f(x, y); returns the number
 * found (may exceed cap), -1 on a CV_Assert condition / bad argument / no memory.  n_cand (optional): the candidates of step 5.
 * The steps are literal about SIGN: a Harris map is negative on edges and may be negative everywhere. */
int crr_detect(const uint8_t *img, int w, int h, int stride, const uint8_t *mask, int mask_stride, int max_corners, double quality_level,
               double min_distance, int block, int harris, double k, float *pts, int cap, int *n_cand, int trap)
{
    if (!(quality_level > 0) || !(min_distance >= 0) || max_corners < 0 || cap < 0 || (cap > 0 && !pts) || (mask && mask_stride < w))
        return -1;
    const size_t n = (size_t)w * h;
    float *eig = (float *)malloc(sizeof(float) * n);
    int *cand = (int *)malloc(sizeof(int) * n);
    if (!eig || !cand || crr_map(img, w, h, stride, block, harris, k, eig, trap, 0, 0) != 0) {
        free(eig);
        free(cand);
        return -1;
    }
    /* Step 4: minMaxLoc(eig, 0, &maxVal, 0, 0, mask): the maximum over the ALLOWED pixels of the whole map, border included; with
     * none allowed maxVal stays 0.  threshold(eig, eig, maxVal * qualityLevel, 0, THRESH_TOZERO): the product in double, thresh cast
     * to the map's f32, dst = src > thresh ? src : 0 on the whole, unmasked map.  With a negative maxVal the threshold lies above it
     * for qualityLevel < 1 (everything becomes 0) and below it for qualityLevel > 1 (negative values survive as they are). */
    double max_val = 0;
    int any = 0;
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            if (mask && !mask[(size_t)y * mask_stride + x])
                continue;
            const float v = eig[(size_t)y * w + x];
            if (!any || v > max_val)
                max_val = v;
            any = 1;
        }
    const float thresh = (float)(max_val * quality_level);
    for (size_t i = 0; i < n; i++)
        eig[i] = eig[i] > thresh ? eig[i] : 0.f;
    /* Step 5: dilate(eig, tmp, Mat()) = 3 x 3 maximum (its constant border is the lowest value: it never wins); candidates are
     * val != 0 && val == tmp (&& mask != 0) for 1 <= y < h - 1, 1 <= x < w - 1, row-major.  Plateau ties are all candidates.  A
     * zeroed neighbour beats a surviving NEGATIVE value, as upstream: 0 is what the threshold wrote there. */
    int nc = 0;
    for (int y = 1; y < h - 1; y++)
        for (int x = 1; x < w - 1; x++) {
            float m = eig[(size_t)y * w + x];
            for (int j = -1; j <= 1; j++)
                for (int i = -1; i <= 1; i++)
                    m = eig[(size_t)(y + j) * w + x + i] > m ? eig[(size_t)(y + j) * w + x + i] : m;
            const float v = eig[(size_t)y * w + x];
            if (v != 0 && v == m && (!mask || mask[(size_t)y * mask_stride + x]))
                cand[nc++] = y * w + x;
        }
    if (n_cand)
        *n_cand = nc;
    /* Step 6: std::sort(tmpCorners, greaterThanPtr()).  The keys are unique, so any correct sort gives this order. */
    g_base = eig;
    qsort(cand, (size_t)nc, sizeof(int), by_quality);
    /* Step 7 */
    int found = 0;
    if (min_distance >= 1) {
        const int cell = (int)lrint(min_distance); /* cvRound: half to even */
        const int gw = (w + cell - 1) / cell, gh = (h + cell - 1) / cell;
        const double md2 = min_distance * min_distance;
        /* the grid's per-cell vectors as linked lists through `next` */
        int *head = (int *)malloc(sizeof(int) * (size_t)gw * gh), *next = (int *)malloc(sizeof(int) * (size_t)(nc + 1));
        if (!head || !next) {
            free(head);
            free(next);
            free(eig);
            free(cand);
            return -1;
        }
        for (int i = 0; i < gw * gh; i++)
            head[i] = -1;
        for (int i = 0; i < nc; i++) {
            const int y = cand[i] / w, x = cand[i] % w;
            const int xc = x / cell, yc = y / cell;
            int x1 = xc - 1, y1 = yc - 1, x2 = xc + 1, y2 = yc + 1;
            x1 = x1 < 0 ? 0 : x1;
            y1 = y1 < 0 ? 0 : y1;
            x2 = x2 > gw - 1 ? gw - 1 : x2;
            y2 = y2 > gh - 1 ? gh - 1 : y2;
            int good = 1;
            for (int yy = y1; yy <= y2 && good; yy++)
                for (int xx = x1; xx <= x2 && good; xx++)
                    for (int j = head[yy * gw + xx]; j >= 0; j = next[j]) {
                        const float dx = (float)x - (float)(cand[j] % w), dy = (float)y - (float)(cand[j] / w);
                        if (dx * dx + dy * dy < md2) { /* (f32 sum of integers, exact; compared as double like upstream) */
                            good = 0;
                            break;
                        }
                    }
            if (good) {
                next[i] = head[yc * gw + xc];
                head[yc * gw + xc] = i;
                if (found < cap) {
                    pts[2 * found] = (float)x;
                    pts[2 * found + 1] = (float)y;
                }
                found++;
                if (max_corners > 0 && found == max_corners)
                    break;
            }
        }
        free(head);
        free(next);
    } else {
        for (int i = 0; i < nc; i++) {
            if (found < cap) {
                pts[2 * found] = (float)(cand[i] % w);
                pts[2 * found + 1] = (float)(cand[i] / w);
            }
            found++;
            if (max_corners > 0 && found == max_corners)
                break;
        }
    }
    free(eig);
    free(cand);
    return found;
}
