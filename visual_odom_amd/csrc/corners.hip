// corners.hip -- the Shi-Tomasi detector of include/vo_corners.h: cv::cornerMinEigenVal(img, eig, 3, 3) and
// cv::goodFeaturesToTrack(img, pts, maxCorners, qualityLevel, minDistance, noArray(), 3, false, 0.04) of OpenCV 4.5 on the level-0
// image of the image table, bit for bit what tests/host_check/corners_ref.c restates from upstream.
//
//   corn_map_kernel      one thread per image column, walking down it: the quality map in upstream's own summation order, and its
//                        maximum (minMaxLoc) by one atomicMax per workgroup
//   corn_cand_kernel     one workgroup per 64 x 16 tile of the map: threshold(TOZERO) at (float)(max * qualityLevel), dilate 3 x 3,
//                        candidates `val != 0 && val == dilated` appended to the image's list as (ordered quality bits, y w + x)
//   corn_select_kernel   one workgroup per image: sort, minDistance suppression, the corners in order
// and goodFeaturesToTrack's mask argument (include/vo_corners_mask.h): the map kernel's masked twin takes the maximum over the allowed
// pixels, the candidate kernel drops the masked-out local maxima, and
//   corn_disc_kernel     one wavefront per kept point: zeros over its disc in a mask that holds 0xFF
// and goodFeaturesToTrack's blockSize, useHarrisDetector and k (include/vo_corners_response.h; tests/host_check/corners_response_ref.c):
//   corn_map_resp_kernel<B, HARRIS>  the map kernel at blockSize 5 and / or with calcHarris's response, masked or not; the
//                        candidate and select kernels take whatever map comes in, negative values included
// and the FRAMES form of the three passes for the frame loop (include/vo_detector.h):
//   corn_map_frames_kernel<B, HARRIS>, corn_cand_frames_kernel, corn_select_frames_kernel
//                        slot = frame, image = quads[frame].l0; a frame whose detect flag is 0 leaves all three at once and reports
//                        no corner; a candidate list beyond lcap is reported as lcap + 1 corners, the count bucket_kernel's split
//                        form turns into the frame's overflow flag.  The bodies are the ones above.
// and the frame loop's top-up under a mask of the carried points (include/vo_topup.h): the map pass above with a null
// max_key, then
//   corn_disc_frames_kernel  corn_disc_kernel's body over the frames' carried lists, the counts read on the device
//   corn_max_frames_kernel   minMaxLoc's masked maximum of the stored map: a flat reduction over w h floats and w h mask bytes
// and the candidate and select kernels of the frames form, the first with a.masks set.
//
// Why a thread per column.  boxFilter sums the f32 products in f64, and its column pass (ColumnSum<double, float>) is a RUNNING sum
// down the whole column: SUM += row(y + 1); out = SUM; SUM -= row(y - 1).  The f64 operations are not exact in general -- a dy of
// one ulp gives a product 70 bits under the sum's top bit -- and an inexact step leaves a residual in SUM that every row below
// inherits (about 1e-19 in a flat region under a textured one, where the plain three-term sum gives 0).  So the sum is not
// order-free, and the kernel sums in upstream's order, which is serial in y.  The columns of 256 images are 318 k threads.
//
// The candidate test is upstream's literally (thresholded value against the 3 x 3 maximum of thresholded values) on the stored map,
// so the candidate list is upstream's own tmpCorners and needs no argument about non-positive values.
//
// Pixels are fetched with REFLECT_101 index arithmetic on the image's own w x h, not from the bordered level: the border is filled by
// the pyramid stage, and this detector runs on an image that has been uploaded and nothing else (a "stale" image of the batch API
// is fine here).  Every load stays inside rows 0 .. h - 1, columns 0 .. w - 1.
//
// Numerics (no FMA contraction: -ffp-contract=off, as the emulator build): Sobel as upstream's separable f32 filter with the scale
// folded into the smoothing taps, products in f32, row sums (c(x-1) + c(x)) + c(x+1) in f64 (RowSum's ksize == 3 branch), the running
// column sum, one cast to f32.  The box sum's border samples are the COV image reflected -- the cov of the reflected POSITION --
// never cov of the reflected source (dx changes sign under reflection, so dx dy would).
#include "vo_corners_dev.h"

namespace vo {

constexpr int CM_T = 256;                         // map kernels: threads per workgroup = cov columns it computes
constexpr int CM_COLS = CM_T - 2;                 // ... columns a workgroup owns at blockSize 3 (+ one halo column each side)
constexpr int CM_COLS5 = CM_T - 4;                // ... at blockSize 5 (+ two)
constexpr int CT_W = 64, CT_H = 16;               // candidate kernel: tile
constexpr int CV_W = CT_W + 2, CV_H = CT_H + 2;   // ... and its values: + the 3 x 3 neighbours of the tile's pixels
constexpr int CORN_SELECT_THREADS = 1024;

__device__ __forceinline__ int corn_clamp(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// The body of the map kernels.  mask: the slot's mask (rows mask_pitch bytes apart) or null.  minMaxLoc(eig, 0, &maxVal, 0, 0,
// mask) takes the maximum over the allowed pixels only (none: max_key stays 0); the map itself is the same with and without one.
//
// B: blockSize, 3 or 5 -- the two sizes for which RowSum<float, double> sums the casts left to right (every other size keeps a
// running sum along the row, which is another kernel).  R = B / 2 halo columns on each side, cov rows -R .. h - 1 + R, and the
// B - 1 row sums that ColumnSum<double, float> still has to subtract in `ring`, oldest first: registers, shifted once per row (at
// B = 5 that is 12 doubles; in LDS they would cost 24 KiB per workgroup and an address per access).  HARRIS: calcHarris in place of
// calcMinEigenVal; k is read by it alone.  (3, false) is cv::cornerMinEigenVal(img, eig, 3, 3) as it always was.
template <int B, int HARRIS>
__device__ __forceinline__ void corn_map_body(const PyrImage *__restrict__ imgs, int image, float *__restrict__ maps, size_t map_stride,
                                              unsigned *__restrict__ max_key, const uint8_t *__restrict__ mask, int mask_pitch, double k)
{
    static_assert(B == 3 || B == 5, "RowSum's left-to-right branches");
    constexpr int R = B / 2, COLS = B == 5 ? CM_COLS5 : CM_COLS;
    __shared__ float s_cov[3][CM_T];
    __shared__ unsigned s_max;
    const int tid = threadIdx.x, slot = blockIdx.y;
    const PyrImage &im = imgs[image];
    const int w = im.w[0], h = im.h[0], stride = im.stride[0];
    const VO_GLOBAL uint8_t *__restrict__ src = (const VO_GLOBAL uint8_t *)im.lvl[0];
    float *__restrict__ map = maps + (size_t)slot * map_stride;
    // this thread's cov column: x of the COV image, which outside the image is the cov of the reflected position rx (boxFilter
    // reflects the cov image); its Sobel reads the source around rx, reflected in turn
    const int x = (int)blockIdx.x * COLS - R + tid;
    const int rx = reflect101(corn_clamp(x, -R, w - 1 + R), w), xa = reflect101(rx - 1, w), xc = reflect101(rx + 1, w);
    const bool owner = tid >= R && tid < CM_T - R && x < w; // (x >= 0 then)
    if (tid == 0)
        s_max = 0;
    const float sf = (float)(1.0 / (255.0 * 4.0 * B)), sf2 = sf * 2.f;
    double sum[3] = {0, 0, 0}, ring[B - 1][3] = {}; // SUM, row(y - R) .. row(y + R - 1) of ColumnSum
    unsigned best = 0;
    for (int yy = -R; yy <= h - 1 + R; yy++) { // cov row yy enters the column sum; the map row yy - R leaves it
        const int ry = reflect101(yy, h);
        // the mask byte of the map row this iteration completes: one coalesced byte per pixel beside the 4-byte store, fetched with
        // the iteration's pixels.  It is a fourth row stream and, unlike two of the three pixel rows, never a cache hit: the masked
        // kernel takes 0.67 ms where the plain one takes 0.53 (256 images of 1241 x 376)
        uint8_t allowed = 1;
        if (mask && owner && yy >= R)
            allowed = mask[(size_t)(yy - R) * mask_pitch + x];
        float rd[3], rs[3];
        for (int j = 0; j < 3; j++) { // RowFilter<uchar, float>: s = k0 p(x-1); s += k1 p(x); s += k2 p(x+1)
            const VO_GLOBAL uint8_t *row = src + (ptrdiff_t)reflect101(ry + j - 1, h) * stride;
            const float pa = (float)row[xa], pb = (float)row[rx], pc = (float)row[xc];
            float s = -1.f * pa;
            s += 0.f * pb;
            s += 1.f * pc;
            rd[j] = s;
            s = sf * pa;
            s += sf2 * pb;
            s += sf * pc;
            rs[j] = s;
        }
        const float dx = (rd[0] + rd[2]) * sf + rd[1] * sf2; // SymmColumnSmallFilter, symmetric
        const float dy = rs[2] - rs[0];                      // ... and its [-1, 0, 1] branch
        s_cov[0][tid] = dx * dx;
        s_cov[1][tid] = dx * dy;
        s_cov[2][tid] = dy * dy;
        __syncthreads();
        double r[3] = {0, 0, 0};
        if (owner)
            for (int c = 0; c < 3; c++) { // RowSum<float, double>, the ksize == 3 and ksize == 5 branches: the casts, left to right
                r[c] = ((double)s_cov[c][tid - R] + (double)s_cov[c][tid - R + 1]) + (double)s_cov[c][tid - R + 2];
                if constexpr (B == 5)
                    r[c] = (r[c] + (double)s_cov[c][tid + 1]) + (double)s_cov[c][tid + 2];
            }
        __syncthreads();
        if (!owner)
            continue;
        if (yy < R) { // SUM = 0; SUM += row(-R); ... SUM += row(R - 1)
            for (int c = 0; c < 3; c++) {
                sum[c] += r[c];
                for (int i = 0; i < B - 2; i++)
                    ring[i][c] = ring[i + 1][c];
                ring[B - 2][c] = r[c];
            }
            continue;
        }
        float box[3];
        for (int c = 0; c < 3; c++) { // s0 = SUM + row(y + R); D = (float)s0; SUM = s0 - row(y - R)
            const double s0 = sum[c] + r[c];
            box[c] = (float)s0;
            sum[c] = s0 - ring[0][c];
            for (int i = 0; i < B - 2; i++)
                ring[i][c] = ring[i + 1][c];
            ring[B - 2][c] = r[c];
        }
        float e;
        if constexpr (HARRIS) { // calcHarris: (float)(a * c - b * b - k * (a + c) * (a + c)), a, b, c floats and k a double
            const float ha = box[0], hb = box[1], hc = box[2];
            e = (float)((double)(ha * hc - hb * hb) - k * (double)(ha + hc) * (double)(ha + hc));
        } else { // calcMinEigenVal
            const float ea = box[0] * 0.5f, eb = box[1], ec = box[2] * 0.5f;
            e = (ea + ec) - sqrtf((ea - ec) * (ea - ec) + eb * eb);
        }
        map[(size_t)(yy - R) * w + x] = e;
        const unsigned key = corn_ord(e);
        if (allowed)
            best = key > best ? key : best;
    }
    if (!max_key) // (uniform)
        return;
    if (best)
        atomicMax(&s_max, best);
    __syncthreads();
    if (tid == 0 && s_max)
        atomicMax(&max_key[slot], s_max);
}

// map: [n][map_stride] floats, slot s = image first + s, rows tight (w floats).  max_key: [n] or null.
__global__ __launch_bounds__(CM_T) void corn_map_kernel(const PyrImage *__restrict__ imgs, int first, float *__restrict__ maps, size_t map_stride,
                                                        unsigned *__restrict__ max_key)
{
    corn_map_body<3, 0>(imgs, first + (int)blockIdx.y, maps, map_stride, max_key, nullptr, 0, 0.0);
}

// ... under masks [n] (CornArgs::masks: a slot's entry may be null)
__global__ __launch_bounds__(CM_T) void corn_map_masked_kernel(const PyrImage *__restrict__ imgs, int first, float *__restrict__ maps, size_t map_stride,
                                                               unsigned *__restrict__ max_key, const uint8_t *const *__restrict__ masks, int mask_pitch)
{
    corn_map_body<3, 0>(imgs, first + (int)blockIdx.y, maps, map_stride, max_key, masks[blockIdx.y], mask_pitch, 0.0);
}

// The response maps of include/vo_corners_response.h: cornerMinEigenVal at blockSize 5, cornerHarris at 3 and 5.  masks: null, or
// as above.  k is an argument, not an instantiation: any finite double.
template <int B, int HARRIS>
__global__ __launch_bounds__(CM_T) void corn_map_resp_kernel(const PyrImage *__restrict__ imgs, int first, float *__restrict__ maps, size_t map_stride,
                                                             unsigned *__restrict__ max_key, const uint8_t *const *__restrict__ masks, int mask_pitch,
                                                             double k)
{
    corn_map_body<B, HARRIS>(imgs, first + (int)blockIdx.y, maps, map_stride, max_key, masks ? masks[blockIdx.y] : nullptr, mask_pitch, k);
}

// The frames form (include/vo_detector.h): slot = frame, its image the left t0 image of the frame's quadruple -- what FAST reads in
// the same call.  detect: null (every frame), or the frames' flags as seq_prepare_kernel / the host wrote them; a frame that does
// not detect again costs the launch of its workgroups and nothing else.  (3, 0) is corn_map_kernel's body.
template <int B, int HARRIS>
__global__ __launch_bounds__(CM_T) void corn_map_frames_kernel(const PyrImage *__restrict__ imgs, const Quad *__restrict__ quads, const int *__restrict__ detect,
                                                               float *__restrict__ maps, size_t map_stride, unsigned *__restrict__ max_key, double k)
{
    if (detect && !detect[blockIdx.y]) // (uniform)
        return;
    corn_map_body<B, HARRIS>(imgs, quads[blockIdx.y].l0, maps, map_stride, max_key, nullptr, 0, k);
}

__device__ __forceinline__ void corn_cand_body(int w, int h, int tiles_x, const CornArgs &a)
{
    __shared__ float s_val[CV_H * CV_W];
    __shared__ unsigned long long s_list[CT_W * CT_H];
    __shared__ int s_cnt, s_base;
    const int tid = threadIdx.x, slot = blockIdx.y;
    const int x0 = (int)(blockIdx.x % (unsigned)tiles_x) * CT_W, y0 = (int)(blockIdx.x / (unsigned)tiles_x) * CT_H;
    const float *__restrict__ map = a.maps + (size_t)slot * a.map_stride;
    if (tid == 0)
        s_cnt = 0;
    // the map at x0 - 1 .. x0 + 64, y0 - 1 .. y0 + 16, clamped into the image (a clamped value is never a candidate's neighbour)
    for (int i = tid; i < CV_H * CV_W; i += 256)
        s_val[i] = map[(size_t)corn_clamp(y0 - 1 + i / CV_W, 0, h - 1) * w + corn_clamp(x0 - 1 + i % CV_W, 0, w - 1)];
    __syncthreads();
    const uint8_t *__restrict__ mask = a.masks ? a.masks[slot] : nullptr; // (uniform)
    // minMaxLoc's maxVal is a double (0 under a mask that allows no pixel); threshold() casts the product to the map's type
    const unsigned mk = a.max_key[slot];
    const float thresh = (float)((double)(mk ? corn_unord(mk) : 0.f) * a.quality);
    for (int i = tid; i < CT_W * CT_H; i += 256) {
        const int lx = i % CT_W, ly = i / CT_W, x = x0 + lx, y = y0 + ly;
        if (x < 1 || x > w - 2 || y < 1 || y > h - 2)
            continue;
        const float *q = s_val + ly * CV_W + lx; // top-left neighbour
        const float v = q[CV_W + 1] > thresh ? q[CV_W + 1] : 0.f;
        if (v == 0.f)
            continue;
        float m = v;
        for (int j = 0; j < 3; j++)
            for (int k = 0; k < 3; k++) {
                const float t = q[j * CV_W + k] > thresh ? q[j * CV_W + k] : 0.f;
                m = t > m ? t : m;
            }
        // the mask is read for the pixels that passed only (a few thousand per image), before the append: a masked-out pixel
        // never enters tmpCorners, but it has taken part in the threshold and the dilate above like any other
        if (v == m && (!mask || mask[(size_t)y * a.mask_pitch + x]))
            s_list[atomicAdd(&s_cnt, 1)] =((unsigned long long)corn_ord(v) << 32) | (unsigned)(y * w + x);
    }
    __syncthreads();
    if (tid == 0)
        s_base = s_cnt ? atomicAdd(&a.ncand[slot], s_cnt) : 0;
    __syncthreads();
    unsigned long long *keys = a.keys + (size_t)slot * a.kcap;
    for (int i = tid; i < s_cnt; i += 256)
        if (s_base + i < a.lcap)
            keys[s_base + i] = s_list[i];
}

__global__ __launch_bounds__(256) void corn_cand_kernel(int w, int h, int tiles_x, CornArgs a) { corn_cand_body(w, h, tiles_x, a); }

// ... of the frames form: detect as in corn_map_frames_kernel
__global__ __launch_bounds__(256) void corn_cand_frames_kernel(int w, int h, int tiles_x, CornArgs a, const int *__restrict__ detect)
{
    if (detect && !detect[blockIdx.y]) // (uniform)
        return;
    corn_cand_body(w, h, tiles_x, a);
}

// bitonic sort of keys[0 .. n), n a power of two, by the whole workgroup (every key is distinct)
__device__ void corn_sort(unsigned long long *keys, int n, bool descending)
{
    const int tid = threadIdx.x, T = blockDim.x;
    for (int k = 2; k <= n; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < n / 2; t += T) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const unsigned long long ki = keys[i], kl = keys[l];
                const bool up = ((i & k) == 0) != descending; // this pair belongs to an ascending run
                if ((ki > kl) == up) {
                    keys[i] = kl;
                    keys[l] = ki;
                }
            }
            __syncthreads();
        }
}

// The rest of goodFeaturesToTrack for one image per workgroup.
//   sort        std::sort with greaterThanPtr = descending by (quality, address): the 64-bit keys, which are distinct.
//   suppression upstream's loop walks the sorted list and accepts a candidate iff no ACCEPTED candidate before it lies in the 3 x 3
//               cells around its own closer than minDistance.  That is the lexicographically first maximal independent set of the
//               conflict relation (same 3 x 3 cell neighbourhood and dx^2 + dy^2 < minDistance^2, symmetric), computed in rounds:
//               an undecided candidate is rejected once a better conflicting one is accepted, accepted once every better
//               conflicting one is rejected.  The best undecided candidate is decided in every round, so the loop ends; decisions
//               are final and each is the serial loop's, by induction over the rank.  A round reads only decisions of EARLIER
//               rounds (status carries the round), so the round count is a property of the input: the depth of its dependency chain.
//   cells       found through a second sorted list (cell, rank): the three cell rows around a candidate are three contiguous
//               ranges of it, each by one binary search.  O(candidates) memory whatever the cell size.
//   maxCorners  the loop stops at maxCorners accepted = the first maxCorners accepted in rank order.
//   overflow    what nout reports for a candidate list beyond lcap: -1 in the detector's own calls (the host answers
//               VO_ERR_OVERFLOW), lcap + 1 in the frames form
__device__ __forceinline__ void corn_select_body(const CornArgs &a, int w, int h, int overflow)
{
    __shared__ int s_part[CORN_SELECT_THREADS];
    __shared__ int s_flag[3];
    const int tid = threadIdx.x, T = blockDim.x, slot = blockIdx.x;
    const int n = a.ncand[slot];
    if (n > a.lcap) { // (uniform) nothing is silently truncated: the host reports VO_ERR_OVERFLOW
        if (tid == 0) {
            a.nout[slot] = overflow;
            if (a.rounds)
                a.rounds[slot] = 0;
        }
        return;
    }
    unsigned long long *keys = a.keys + (size_t)slot * a.kcap, *ckeys = a.ckeys + (size_t)slot * a.kcap;
    int *st = a.status + (size_t)slot * a.lcap;
    float2 *pts = a.pts + (size_t)slot * a.lcap;
    int np = 1;
    while (np < n)
        np <<= 1;
    for (int i = n + tid; i < np; i += T)
        keys[i] = 0; // (below every key: corn_ord is never 0 for a value that passed the threshold)
    __syncthreads();
    corn_sort(keys, np, true);
    const int limit = a.max_corners > 0 && a.max_corners < n ? a.max_corners : n;
    if (a.lim <= 1) { // minDistance < 1, or so small that no two pixels conflict: the first maxCorners of the list
        for (int i = tid; i < limit; i += T) {
            const int idx = (int)(unsigned)keys[i];
            pts[i] = make_float2((float)(idx % w), (float)(idx / w));
        }
        if (tid == 0) {
            a.nout[slot] = limit;
            if (a.rounds)
                a.rounds[slot] = 0;
        }
        return;
    }
    const int cell = a.cell, gw = (w + cell - 1) / cell, gh = (h + cell - 1) / cell;
    for (int i = tid; i < np; i += T) {
        if (i < n) {
            const int idx = (int)(unsigned)keys[i];
            ckeys[i] = ((unsigned long long)(unsigned)((idx / w) / cell * gw + (idx % w) / cell) << 32) | (unsigned)i;
            st[i] = 0;
        } else
            ckeys[i] = ~0ull;
    }
    if (tid < 3)
        s_flag[tid] = 0;
    __syncthreads();
    corn_sort(ckeys, np, false);
    int round = 0;
    for (;;) {
        round++;
        if (tid == 0)
            s_flag[(round + 1) % 3] = 0; // (read last in round - 2)
        bool left = false;
        for (int i = tid; i < n; i += T) {
            if (st[i] != 0) // (st is read and written by different threads inside a round without atomics, on purpose: an aligned
                continue;   // int is never torn, and the round stamp makes a value written in this round read as "undecided")
            const int idx = (int)(unsigned)keys[i], x = idx % w, y = idx / w, xc = x / cell, yc = y / cell;
            const int c0 = xc > 0 ? xc - 1 : 0, c1 = xc < gw - 1 ? xc + 1 : gw - 1;
            int verdict = 1; // 1 accept, 0 reject, -1 wait
            for (int yy = (yc > 0 ? yc - 1 : 0); yy <= (yc < gh - 1 ? yc + 1 : gh - 1) && verdict != 0; yy++) {
                const unsigned long long lo_key = (unsigned long long)(unsigned)(yy * gw + c0) << 32;
                const unsigned hi_cell = (unsigned)(yy * gw + c1);
                int lo = 0, hi = n; // first entry >= lo_key
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (ckeys[mid] < lo_key)
                        lo = mid + 1;
                    else
                        hi = mid;
                }
                for (int p = lo; p < n; p++) {
                    const unsigned long long ck = ckeys[p];
                    if ((unsigned)(ck >> 32) > hi_cell)
                        break;
                    const int j = (int)(unsigned)ck;
                    if (j >= i)
                        continue;
                    const int jdx = (int)(unsigned)keys[j], ddx = x - jdx % w, ddy = y - jdx / w;
                    if (ddx * ddx + ddy * ddy >= a.lim)
                        continue;
                    const int sj = st[j];
                    if (sj == 0 || (sj >> 1) >= round)
                        verdict = -1; // undecided before this round
                    else if (sj & 1) {
                        verdict = 0;
                        break;
                    }
                }
            }
            if (verdict >= 0)
                st[i] = round << 1 | verdict;
            else
                left = true;
        }
        if (left)
            s_flag[round % 3] = 1;
        __syncthreads();
        if (!s_flag[round % 3])
            break;
    }
    // one scan over the rank-ordered accept flags: contiguous chunks, chunk totals through LDS
    const int chunk = (n + T - 1) / T, b = tid * chunk < n ? tid * chunk : n, e = b + chunk < n ? b + chunk : n;
    int mine = 0;
    for (int i = b; i < e; i++)
        mine += st[i] & 1;
    s_part[tid] = mine;
    __syncthreads();
    int off = 0, total = 0;
    for (int t = 0; t < T; t++) {
        off += t < tid ? s_part[t] : 0;
        total += s_part[t];
    }
    const int cut = a.max_corners > 0 && a.max_corners < total ? a.max_corners : total;
    for (int i = b; i < e; i++)
        if (st[i] & 1) {
            if (off < cut) {
                const int idx = (int)(unsigned)keys[i];
                pts[off] = make_float2((float)(idx % w), (float)(idx / w));
            }
            off++;
        }
    if (tid == 0) {
        a.nout[slot] = cut;
        if (a.rounds)
            a.rounds[slot] = round;
    }
}

__global__ __launch_bounds__(CORN_SELECT_THREADS) void corn_select_kernel(CornArgs a, int w, int h) { corn_select_body(a, w, h, -1); }

// ... of the frames form: a.pts / a.nout are the frame loop's corner list and count ([frames][lcap] and [frames], the layout of
// bucket_kernel's split form).  A frame that does not detect again appends nothing: nout = 0.  A candidate list beyond lcap comes out
// as lcap + 1 corners: no list holds that many, so seq_prepare_kernel hands the count on as it is and bucket_kernel's `n_new > cap`
// sets bit 0 of the frame's overflow flag -- the way a FAST list that did not fit is reported.
__global__ __launch_bounds__(CORN_SELECT_THREADS) void corn_select_frames_kernel(CornArgs a, int w, int h, const int *__restrict__ detect)
{
    if (detect && !detect[blockIdx.x]) { // (uniform)
        if (threadIdx.x == 0) {
            a.nout[blockIdx.x] = 0;
            if (a.rounds)
                a.rounds[blockIdx.x] = 0;
        }
        return;
    }
    corn_select_body(a, w, h, a.lcap + 1);
}

// The disc mask of include/vo_corners_mask.h over a mask that holds 0xFF: one wavefront per kept point writes zeros over the part of
// its disc that lies inside the image.  Centre (cvRound(x), cvRound(y)), round-half-to-even; a point with a NaN, infinite or
// |coordinate| >= 2^30 is skipped; pixel (px, py) is cleared iff (px - cx)^2 + (py - cy)^2 <= radius^2 in integers (inside the clipped
// box both offsets are at most radius <= 256, and cx +- radius stays far inside int).  Every writer stores the same byte, so
// overlapping discs need no atomics and the result does not depend on order.
constexpr int CD_T = 256, CD_WAVES = CD_T / 64;
// kept point p by the calling wavefront (p is uniform per wavefront)
__device__ __forceinline__ void corn_disc_body(const float2 *__restrict__ kept, int n_kept, int p, int radius, uint8_t *__restrict__ mask, int w, int h,
                                               int pitch)
{
    const int lane = (int)threadIdx.x % 64;
    if (p >= n_kept) // (uniform per wavefront)
        return;
    const float2 k = kept[p];
    if (!(fabsf(k.x) < 1073741824.f) || !(fabsf(k.y) < 1073741824.f)) // (NaN fails the comparison too)
        return;
    const int cx = __float2int_rn(k.x), cy = __float2int_rn(k.y);
    const int x0 = cx - radius > 0 ? cx - radius : 0, x1 = cx + radius < w - 1 ? cx + radius : w - 1;
    const int y0 = cy - radius > 0 ? cy - radius : 0, y1 = cy + radius < h - 1 ? cy + radius : h - 1;
    if (x0 > x1 || y0 > y1) // the disc misses the image
        return;
    const int bw = x1 - x0 + 1, cells = bw * (y1 - y0 + 1), r2 = radius * radius;
    for (int i = lane; i < cells; i += 64) {
        const int px = x0 + i % bw, py = y0 + i / bw, dx = px - cx, dy = py - cy;
        if (dx * dx + dy * dy <= r2)
            mask[(size_t)py * pitch + px] = 0;
    }
}

__global__ __launch_bounds__(CD_T) void corn_disc_kernel(const float2 *__restrict__ kept, int n_kept, int radius, uint8_t *__restrict__ mask, int w, int h,
                                                         int pitch)
{
    corn_disc_body(kept, n_kept, (int)blockIdx.x * CD_WAVES + (int)threadIdx.x / 64, radius, mask, w, h, pitch);
}

// The frames form (include/vo_topup.h): the kept list of frame f is the carried set at entry, feat + f * fcap, its count n_tracked[f]
// read here -- in the lock-step loop only the device knows it.  planes[f]: the frame's mask, rows w bytes apart, which a fill on the
// same stream has set to 0xFF.  The grid's x covers the largest carried set that still detects again (redetect_below - 1 points, at
// most fcap); the loop makes a smaller grid right too (grid_x: gridDim.x, as an argument like seq_ingest_kernel's).
__global__ __launch_bounds__(CD_T) void corn_disc_frames_kernel(const float2 *__restrict__ feat, int fcap, const int *__restrict__ n_tracked,
                                                                const int *__restrict__ detect, int radius, uint8_t *const *__restrict__ planes, int w,
                                                                int h, int grid_x /* = the grid's x */)
{
    const int f = blockIdx.y;
    if (detect && !detect[f]) // (uniform)
        return;
    int n = n_tracked[f];
    n = n < fcap ? n : fcap;
    uint8_t *__restrict__ mask = planes[f];
    for (int p = (int)blockIdx.x * CD_WAVES + (int)threadIdx.x / 64; p < n; p += grid_x * CD_WAVES)
        corn_disc_body(feat + (size_t)f * fcap, n, p, radius, mask, w, h, w);
}

// minMaxLoc(eig, 0, &maxVal, 0, 0, mask) of the frames form, on the map the map pass stored: max_key[f] = the largest corn_ord(value)
// over the pixels whose mask byte is non-zero, border rows and columns included, 0 when none is allowed -- the bits corn_map_body
// leaves under the same mask (an integer maximum: exact, so its order is free).
//
// A streaming reduction.  Map rows are tight and the planes have pitch w, so a frame is one flat run of n = w h floats beside n bytes.
// A lane takes four floats by one 16-byte load and their four mask bytes by one 4-byte load, CX_UNROLL such groups a pass with all
// loads issued before the first compare.  The run's start need not be 16-byte aligned (map_stride = max_w max_h floats, any w h):
// the floats in front of the first aligned address and those behind the last whole group go one to a lane of the first workgroup.
// The mask word is then at whatever alignment the plane has beside the map's (an align-1 dword, which global memory takes).
// The wavefront's maximum is taken in registers (DPP: two quad permutes, two mirrors, two row broadcasts; 0 is neutral), the four
// wavefronts meet in LDS once, and one atomicMax per workgroup reaches memory.  No value is kept across frames.
constexpr int CX_T = 256, CX_UNROLL = 4, CX_PER_WG = CX_T * CX_UNROLL * 4; // floats a workgroup takes per pass

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned dpp_umax(unsigned v)
{
    const unsigned o = (unsigned)VO_UPDATE_DPP(0, (int)v, CTRL, ROW_MASK, 0xf, true);
    return o > v ? o : v;
}

__global__ __launch_bounds__(CX_T) void corn_max_frames_kernel(const float *__restrict__ maps, size_t map_stride, const uint8_t *const *__restrict__ planes,
                                                               int n, const int *__restrict__ detect, unsigned *__restrict__ max_key, int grid_x /* = the grid's x */)
{
    __shared__ unsigned s_wave[CX_T / 64];
    const int f = blockIdx.y, tid = threadIdx.x;
    if (detect && !detect[f]) // (uniform)
        return;
    const float *__restrict__ map = maps + (size_t)f * map_stride;
    const uint8_t *__restrict__ mask = planes[f];
    int head = (int)((16u - (unsigned)((uintptr_t)map & 15u)) & 15u) / 4; // floats in front of the first 16-byte boundary
    head = head < n ? head : n;
    const int groups = (n - head) / 4, tail0 = head + groups * 4; // whole groups; the first float behind them
    unsigned best = 0;
    if (blockIdx.x == 0) { // head and tail: at most 3 + 3 single elements
        const int i = tid < head ? tid : tail0 + (tid - head);
        if (i < n && mask[i]) {
            const unsigned key = corn_ord(map[i]);
            best = key;
        }
    }
    const uint4 *__restrict__ m4 = reinterpret_cast<const uint4 *>(map + head);
    const uint8_t *__restrict__ k1 = mask + head;
    for (int g0 = (int)blockIdx.x * (CX_T * CX_UNROLL); g0 < groups; g0 += grid_x * (CX_T * CX_UNROLL)) {
        uint4 v[CX_UNROLL];
        uint32_t k[CX_UNROLL];
        for (int u = 0; u < CX_UNROLL; u++) {
            const int g = g0 + u * CX_T + tid;
            if (g < groups) {
                v[u] = m4[g];
                k[u] = reinterpret_cast<const U32A1 *>(k1 + (size_t)g * 4)->a;
            } else {
                v[u] = make_uint4(0, 0, 0, 0);
                k[u] = 0;
            }
        }
        for (int u = 0; u < CX_UNROLL; u++) {
            if (!k[u])
                continue;
            const uint32_t q[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
            for (int j = 0; j < 4; j++)
                if ((k[u] >> (8 * j)) & 0xffu) {
                    const unsigned key = (q[j] & 0x80000000u) ? ~q[j] : (q[j] | 0x80000000u); // corn_ord on the bits
                    best = key > best ? key : best;
                }
        }
    }
    best = dpp_umax<VO_DPP_QUAD_XOR1, 0xf>(best);
    best = dpp_umax<VO_DPP_QUAD_XOR2, 0xf>(best);
    best = dpp_umax<VO_DPP_ROW_HALF_MIRROR, 0xf>(best);
    best = dpp_umax<VO_DPP_ROW_MIRROR, 0xf>(best);
    best = dpp_umax<VO_DPP_ROW_BCAST15, 0xa>(best);
    best = dpp_umax<VO_DPP_ROW_BCAST31, 0xc>(best); // lane 63 holds the wavefront's maximum
    if (tid % 64 == 63)
        s_wave[tid / 64] = best;
    __syncthreads();
    if (tid == 0) {
        unsigned m = s_wave[0];
        for (int i = 1; i < CX_T / 64; i++)
            m = s_wave[i] > m ? s_wave[i] : m;
        if (m)
            atomicMax(&max_key[f], m);
    }
}

#ifndef VO_HOST_EMUL
// the map pass of a response other than (3, min-eigen): masks may be null
template <int B, int HARRIS>
static void launch_resp_map(const PyrImage *d_imgs, int first, int n, int w, float *maps, size_t map_stride, unsigned *max_key,
                            const uint8_t *const *masks, int mask_pitch, double k, hipStream_t stream)
{
    constexpr int COLS = CM_T - 2 * (B / 2);
    hipLaunchKernelGGL((corn_map_resp_kernel<B, HARRIS>), dim3((w + COLS - 1) / COLS, n), dim3(CM_T), 0, stream, d_imgs, first, maps, map_stride, max_key, masks,
                       mask_pitch, k);
}

static void launch_resp_map(int block_size, int use_harris, const PyrImage *d_imgs, int first, int n, int w, float *maps, size_t map_stride,
                            unsigned *max_key, const uint8_t *const *masks, int mask_pitch, double k, hipStream_t stream)
{
    if (block_size == 5 && !use_harris)
        launch_resp_map<5, 0>(d_imgs, first, n, w, maps, map_stride, max_key, masks, mask_pitch, k, stream);
    else if (block_size == 5)
        launch_resp_map<5, 1>(d_imgs, first, n, w, maps, map_stride, max_key, masks, mask_pitch, k, stream);
    else
        launch_resp_map<3, 1>(d_imgs, first, n, w, maps, map_stride, max_key, masks, mask_pitch, k, stream);
}

hipError_t launch_corners(const PyrImage *d_imgs, int first, int n, int w, int h, const CornArgs &a, hipStream_t stream)
{
    if (n <= 0)
        return hipSuccess;
    hipError_t e = hipMemsetAsync(a.max_key, 0, sizeof(unsigned) * (size_t)n, stream);
    if (e == hipSuccess)
        e = hipMemsetAsync(a.ncand, 0, sizeof(int) * (size_t)n, stream);
    if (e != hipSuccess)
        return e;
    const int tiles_x = (w + CT_W - 1) / CT_W, tiles_y = (h + CT_H - 1) / CT_H;
    if (a.block_size != 3 || a.use_harris)
        launch_resp_map(a.block_size, a.use_harris, d_imgs, first, n, w, a.maps, a.map_stride, a.max_key, a.masks, a.mask_pitch, a.harris_k, stream);
    else if (a.masks)
        hipLaunchKernelGGL(corn_map_masked_kernel, dim3((w + CM_COLS - 1) / CM_COLS, n), dim3(CM_T), 0, stream, d_imgs, first, a.maps, a.map_stride, a.max_key,
                           a.masks, a.mask_pitch);
    else
        hipLaunchKernelGGL(corn_map_kernel, dim3((w + CM_COLS - 1) / CM_COLS, n), dim3(CM_T), 0, stream, d_imgs, first, a.maps, a.map_stride, a.max_key);
    hipLaunchKernelGGL(corn_cand_kernel,dim3(tiles_x * tiles_y, n), dim3(256), 0, stream, w, h, tiles_x, a);
    hipLaunchKernelGGL(corn_select_kernel, dim3(n), dim3(CORN_SELECT_THREADS), 0, stream, a, w, h);
    return hipGetLastError();
}

template <int B, int HARRIS>
static void launch_frames_map(const PyrImage *d_imgs, const Quad *d_quads, const int *d_detect, int n, int w, const CornArgs &a, unsigned *max_key,
                              hipStream_t stream)
{
    constexpr int COLS = CM_T - 2 * (B / 2);
    hipLaunchKernelGGL((corn_map_frames_kernel<B, HARRIS>), dim3((w + COLS - 1) / COLS, n), dim3(CM_T), 0, stream, d_imgs, d_quads, d_detect, a.maps,
                       a.map_stride, max_key, a.harris_k);
}

// max_key: a.max_key, or null for the map alone (the top-up's split: corn_max_frames_kernel takes the maximum under the mask)
static void launch_frames_map(const PyrImage *d_imgs, const Quad *d_quads, const int *d_detect, int n, int w, const CornArgs &a, unsigned *max_key,
                              hipStream_t stream)
{
    if (a.block_size == 5 && !a.use_harris)
        launch_frames_map<5, 0>(d_imgs, d_quads, d_detect, n, w, a, max_key, stream);
    else if (a.block_size == 5)
        launch_frames_map<5, 1>(d_imgs, d_quads, d_detect, n, w, a, max_key, stream);
    else if (a.use_harris)
        launch_frames_map<3, 1>(d_imgs, d_quads, d_detect, n, w, a, max_key, stream);
    else
        launch_frames_map<3, 0>(d_imgs, d_quads, d_detect, n, w, a, max_key, stream);
}

hipError_t launch_corners_frames(const PyrImage *d_imgs, const Quad *d_quads, const int *d_detect, int n, int w, int h, const CornArgs &a, hipStream_t stream)
{
    if (n <= 0)
        return hipSuccess;
    hipError_t e = hipMemsetAsync(a.max_key, 0, sizeof(unsigned) * (size_t)n, stream);
    if (e == hipSuccess)
        e = hipMemsetAsync(a.ncand, 0, sizeof(int) * (size_t)n, stream);
    if (e != hipSuccess)
        return e;
    const int tiles_x = (w + CT_W - 1) / CT_W, tiles_y = (h + CT_H - 1) / CT_H;
    launch_frames_map(d_imgs, d_quads, d_detect, n, w, a, a.max_key, stream);
    hipLaunchKernelGGL(corn_cand_frames_kernel, dim3(tiles_x * tiles_y, n), dim3(256), 0, stream, w, h, tiles_x, a, d_detect);
    hipLaunchKernelGGL(corn_select_frames_kernel, dim3(n), dim3(CORN_SELECT_THREADS), 0, stream, a, w, h, d_detect);
    return hipGetLastError();
}

hipError_t launch_corners_frames_map(const PyrImage *d_imgs, const Quad *d_quads, const int *d_detect, int n, int w, const CornArgs &a, hipStream_t stream)
{
    if (n <= 0)
        return hipSuccess;
    launch_frames_map(d_imgs, d_quads, d_detect, n, w, a, nullptr, stream);
    return hipGetLastError();
}

hipError_t launch_corner_disc_frames(const int *d_detect, int n, int w, int h, const CornTopArgs &t, hipStream_t stream)
{
    if (n <= 0)
        return hipSuccess;
    // the planes' w h bytes each (plane_stride apart)
    hipError_t e = hipMemset2DAsync(t.plane0, t.plane_stride, 0xFF, (size_t)w * h, (size_t)n, stream);
    if (e != hipSuccess)
        return e;
    int kept = t.max_kept < t.fcap ? t.max_kept : t.fcap;
    kept = kept > 0 ? kept : 1;
    const int disc_x = (kept + CD_WAVES - 1) / CD_WAVES;
    hipLaunchKernelGGL(corn_disc_frames_kernel, dim3(disc_x, n), dim3(CD_T), 0, stream, t.feat, t.fcap, t.n_tracked, d_detect, t.radius, t.planes, w, h, disc_x);
    return hipGetLastError();
}

hipError_t launch_corners_frames_masked(const int *d_detect, int n, int w, int h, const CornArgs &a, const CornTopArgs &t, hipStream_t stream)
{
    if (n <= 0)
        return hipSuccess;
    hipError_t e = hipMemsetAsync(a.max_key, 0, sizeof(unsigned) * (size_t)n, stream);
    if (e == hipSuccess)
        e = hipMemsetAsync(a.ncand, 0, sizeof(int) * (size_t)n, stream);
    if (e == hipSuccess)
        e = launch_corner_disc_frames(d_detect, n, w, h, t, stream);
    if (e != hipSuccess)
        return e;
    const int cells = w * h;
    int wgs = (cells + CX_PER_WG - 1) / CX_PER_WG;
    wgs = wgs < 1 ? 1 : wgs > 1024 ? 1024 : wgs;
    hipLaunchKernelGGL(corn_max_frames_kernel, dim3(wgs, n), dim3(CX_T), 0, stream, a.maps, a.map_stride, a.masks, cells, d_detect, a.max_key, wgs);
    const int tiles_x = (w + CT_W - 1) / CT_W, tiles_y = (h + CT_H - 1) / CT_H;
    hipLaunchKernelGGL(corn_cand_frames_kernel, dim3(tiles_x * tiles_y, n), dim3(256), 0, stream, w, h, tiles_x, a, d_detect);
    hipLaunchKernelGGL(corn_select_frames_kernel, dim3(n), dim3(CORN_SELECT_THREADS), 0, stream, a, w, h, d_detect);
    return hipGetLastError();
}

void launch_corner_map(const PyrImage *d_imgs, int image, int w, int h, float *d_map, hipStream_t stream, int block_size, int use_harris, double k)
{
    if (block_size != 3 || use_harris)
        launch_resp_map(block_size, use_harris, d_imgs, image, 1, w, d_map, (size_t)0, (unsigned *)nullptr, (const uint8_t *const *)nullptr, 0, k, stream);
    else
        hipLaunchKernelGGL(corn_map_kernel, dim3((w + CM_COLS - 1) / CM_COLS, 1), dim3(CM_T), 0, stream, d_imgs, image, d_map, (size_t)0, (unsigned *)nullptr);
}

hipError_t launch_corner_disc_mask(const float2 *d_kept, int n_kept, int radius, uint8_t *d_mask, int w, int h, hipStream_t stream)
{
    hipError_t e = hipMemsetAsync(d_mask, 0xFF, (size_t)w * h, stream);
    if (e != hipSuccess || n_kept <= 0)
        return e;
    hipLaunchKernelGGL(corn_disc_kernel, dim3((n_kept + CD_WAVES - 1) / CD_WAVES), dim3(CD_T), 0, stream, d_kept, n_kept, radius, d_mask, w, h, w);
    return hipGetLastError();
}
#endif

} // namespace vo
