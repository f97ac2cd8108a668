// lk.hip -- the pyramidal Lucas-Kanade kernels: the fused 4-hop "circular matching" chain, the same body for a range of its
// hops, and for ONE hop between two images with the err output (the two-image tracker).
//
// Replaces the four chained cv::calcOpticalFlowPyrLK calls of circularMatching()
// (reference src/feature.cpp:136-139: l0->r0, r0->r1, r1->l1, l1->l0; winSize 21x21, maxLevel 3,
// TermCriteria(COUNT+EPS, 30, 0.01), flags 0, minEigThreshold 1e-3, err vector requested).
// Semantics follow OpenCV's CPU LKTrackerInvoker: 14-bit fixed-point bilinear weights, int16
// template (I*32, Scharr Ix/Iy), 2x2 structure tensor, min-eigenvalue test, <=30 Gauss-Newton
// iterations with the eps^2 and oscillation stops, +-winSize admissibility window, final in-bounds
// status check.  The five sums A11/A12/A22/b1/b2 are accumulated exactly in integers (so the result
// does not depend on reduction order) and rounded to f32 once; the 2x2 solve is plain f32 with
// contraction off.
//
// Mapping (CDNA4): ONE WAVEFRONT PER FEATURE, one single-wave workgroup per feature.  A feature is
// a serial chain (4 hops x 4 levels x <=30 iterations) but independent of every other feature, so
// the wave keeps all per-feature state in registers and never synchronises with another wave.
//   lane l -> window row r = l/3, column segment s = l%3 (7 px): 63 lanes cover the 21x21 window.
//   Template: each lane loads its 2 x 8 pixels and 2 x 8 Scharr samples straight from the bordered
//   pyramid (no border path, no staging) and keeps the 7 samples of I, Ix, Iy packed two per VGPR
//   (12 VGPRs) for the whole level.
//   Search image J: a 40 x 48 byte tile in LDS (1920 B per wave), filled with 16-byte loads (two
//   per lane, straight-line: lk_tile_refill_wave) and re-fetched only when the window leaves it; a
//   pixel cell reads two unaligned 8-byte rows once and keeps its 8 columns lifted in registers.
//   Pixel arithmetic: v_perm_b32 / v_dot2_u32_u16 / v_dot2_i32_i16 / v_pk_sub_i16 (vo_lkmath.h), every
//   bilinear sample from VERTICAL pixel pairs (t[k], b[k]) against the weights packed by column: each
//   column is lifted once (8 v_perm_b32 per cell, where horizontal pairs took 14; profiles/r07_lk_vertical_pairs.md).
//   Reductions: v_permlane32/16_swap + v_add_u32_dpp butterflies, two sums per tree (vo_dev.h
//   wave_sum2_exact_f32), no LDS round trips.  A level whose structure tensor says that b1, b2 fit 32 bits (lk_sums_fit,
//   vo_lkmath.h) sums them in one tree of wrapping 32-bit adds instead (wave_sum2_f32; profiles/r11_lk_fit_sums.md); the level's
//   iteration loop exists once per kind of sum, chosen once per level (profiles/r12_lk_iteration_branches.md).
// Grid: blocks are numbered so that (dispatcher: block b -> XCD b % 8) all features of one frame
// run on ONE XCD, i.e. the frame's four pyramids are pulled into one L2 only, eight frames at a time.
// Batches of fewer than 8 frames split each frame's feature list into contiguous parts over 8/fpg XCDs.
// lk_circular_queue_kernel (round 10, batches of 16 frames and more): the same numbering handed out as tickets of per-XCD queues,
// so that an XCD that runs dry takes work from the others (vo_lkqueue.h, profiles/r10_lk_xcd_queue.md).
// lk_hops_kernel (round 6): the same body for hops [begin, end) of the chain -- the synchronous drop-in calls on the kept pair
// launch hop 0 while the new pair is still crossing PCIe (capi_run.hip); lk_circular_kernel is what every other launch runs.
// lk_flow_kernel: the same body for ONE hop between an arbitrary (prev, next) pair of the image table, with the err output of
// cv::calcOpticalFlowPyrLK -- the reference's featureTracking() (feature.cpp:64-74; voflow_*, capi_flow.hip).
// lk_flow_win_kernel<W>: lk_flow_kernel with a W x W window, W odd in 5 .. 19 (vowin_*, include/vo_flow_win.h): the body with the
// window as a template parameter, the lane map of LkWin<W> below.
// lk_flow_flags_kernel<W>: the same hop with the two flags of cv::calcOpticalFlowPyrLK (voflag_*, include/vo_flow_flags.h), every odd
// W of 5 .. 21: the search starts at the caller's guess, err is the min eigenvalue of the level-0 structure tensor.
#include "vo_kernels.h"
#include "vo_lkmath.h"
#include "vo_lkqueue.h"

#include <float.h>
#include <type_traits>

namespace vo {

#ifdef VO_HOST_EMUL
// (the CPU emulator only) iterations run per pyramid level with the 32-bit sums [level][1] and with the split ones [level][0]
inline long long g_lk_fit_iterations[VO_MAX_LEVELS][2];
#define VO_LK_COUNT_FIT(level, fit) ((void)(threadIdx.x == 0 ? ++g_lk_fit_iterations[level][(fit) ? 1 : 0] : 0))
// (the same) iterations that sampled the search window with iw11 = -1, the rare case of blend7_cols (vo_lkmath.h)
inline long long g_lk_neg_iterations;
#define VO_LK_COUNT_NEG(neg) ((void)(threadIdx.x == 0 && (neg) ? ++g_lk_neg_iterations : 0))
#else
#define VO_LK_COUNT_FIT(level, fit) ((void)0)
#define VO_LK_COUNT_NEG(neg) ((void)0)
#endif

constexpr int LK_WIN = 21; // the window of the chain kernels and of lk_flow_kernel; lk_flow_win_kernel<W>: odd W of 5 .. 19
constexpr int LK_JT_W = 48, LK_JT_H = 40; // search tile (bytes x rows), LDS row stride = LK_JT_W
// A W x W window on the wavefront: a row is cut into SEGS 7-pixel segments, lane -> (row = lane / SEGS, segment = lane % SEGS),
// W * SEGS lanes own pixels (63 for W = 21, at most 57 below).  A lane always reads the 8 columns of its segment, so a row of
// the window reads COLS = 7 * SEGS + 1 columns -- W + 1 only where 7 divides W -- and the last segment of a row holds
// LAST = W - 7 * (SEGS - 1) pixels of the window; the rest of it is masked out of every sum (lk_seg_mask).
template <int W>
struct LkWin {
    static_assert(W % 2 == 1 && W >= 5 && W <= LK_WIN, "odd windows of 5 .. 21: the pyramid's borders are laid out for 21");
    static constexpr int SEGS = (W + 6) / 7, LANES = W * SEGS, COLS = 7 * SEGS + 1, ROWS = W + 1, LAST = W - 7 * (SEGS - 1);
    // where a new tile starts relative to the corner: the window's reads centred in the tile (12 and 9 for W = 21)
    static constexpr int OFF_X = ((LK_JT_W - COLS) / 2) & ~3, OFF_Y = (LK_JT_H - ROWS) / 2;
    static_assert(LANES <= 64 && LK_JT_W >= COLS + OFF_X + 3 && LK_JT_H >= ROWS + OFF_Y, "the lane map and the tile hold the window");
};
// the packed int16 pair m (pixels 2 m, 2 m + 1) of a segment that holds `valid` pixels of the window: ones where the pixel counts
constexpr uint32_t lk_seg_mask(int valid, int m)
{
    return (2 * m < valid ? 0x0000ffffu : 0u) | (2 * m + 1 < valid ? 0xffff0000u : 0u);
}

// (the 14-bit fixed-point bilinear weights, lk_weights / lk_weights_cols: vo_lkmath.h)

// ---- the search tile: LK_JT_H rows of LK_JT_W bytes of J in LDS, origin (jx0, jy0) -------------------------------------
// The helpers take and return the origin BY VALUE: a local whose address goes into a call stays in memory until the call is
// inlined, and the kernels' scalar control flow then comes out differently (profiles/kernel_sources.md).
struct LkOrigin {
    int x, y;
};
// is there no tile yet, or does it miss part of what the window of corner (inx, iny) reads: columns inx .. inx + 21, rows
// iny .. iny + 21 (W = 21; in general LkWin<W>::COLS columns, masked ones included, and W + 1 rows)
template <int W = LK_WIN>
__device__ __forceinline__ bool lk_tile_misses(bool have_tile, int jx0, int jy0, int inx, int iny)
{
    return !have_tile || inx < jx0 || inx + LkWin<W>::COLS > jx0 + LK_JT_W || iny < jy0 || iny + LkWin<W>::ROWS > jy0 + LK_JT_H;
}
// the origin of a new tile around corner (inx, iny): 4-byte aligned, clamped to [-VO_BX, jx_max] x [-VO_BY, jy_max], which keeps
// the tile inside the level's rectangle
template <int W = LK_WIN>
__device__ __forceinline__ LkOrigin lk_tile_origin(int jx_max, int jy_max, int inx, int iny)
{
    int jx0 = (inx - LkWin<W>::OFF_X) & ~3;
    int jy0 = iny - LkWin<W>::OFF_Y;
    jx0 = jx0 < -VO_BX ? -VO_BX : jx0 > jx_max ? jx_max : jx0;
    jy0 = jy0 < -VO_BY ? -VO_BY : jy0 > jy_max ? jy_max : jy0;
    return LkOrigin{jx0, jy0};
}
// a new tile around corner (inx, iny): the origin and the fill, 16-byte chunks c0, c0 + step, ... of the tile's
// LK_JT_H * LK_JT_W / 16 (chunk c = 3 row + col lies at LDS byte 16 c).  Returns the origin.  No barrier in here: the caller
// orders the fill against the LDS reads around it.  The general form, for the pair kernel's half waves (dev/lk_dev.hip).
template <int W = LK_WIN>
__device__ __forceinline__ LkOrigin lk_tile_refill(uint8_t *tile, const VO_GLOBAL uint8_t *__restrict__ Jimg, int jstride, int jx_max, int jy_max,
                                               int inx, int iny, int c0, int step)
{
    const LkOrigin org = lk_tile_origin<W>(jx_max, jy_max, inx, iny);
    const int jx0 = org.x, jy0 = org.y;
    const VO_GLOBAL uint8_t *tb = Jimg + (ptrdiff_t)jy0 * jstride + jx0;
    for (int c = c0; c < LK_JT_H * (LK_JT_W / 16); c += step) {
        const int row = c / (LK_JT_W / 16), col = c - row * (LK_JT_W / 16);
        const U32x4A4 v = *(const VO_GLOBAL U32x4A4 *)(tb + (uint32_t)(row * jstride + 16 * col));
        *reinterpret_cast<uint4 *>(&tile[row * LK_JT_W + 16 * col]) = make_uint4(v.a, v.b, v.c, v.d);
    }
    return org;
}
// The same for a whole wave, chunks (lane, lane + 64), as straight-line code: the tile has 120 chunks, so every lane owns chunk
// `lane` and the lanes below 56 a second one, 64 further = 21 rows and one column on (row + 22, column 0 from column 2).  One
// division by 3 per fill instead of one per chunk, and both loads are in flight before the first is waited for.
template <int W = LK_WIN>
__device__ __forceinline__ LkOrigin lk_tile_refill_wave(uint8_t *tile, const VO_GLOBAL uint8_t *__restrict__ Jimg, int jstride, int jx_max,
                                                    int jy_max, int inx, int iny, int lane)
{
    constexpr int CPR = LK_JT_W / 16, CHUNKS = LK_JT_H * CPR; // chunks per row, chunks
    static_assert(CPR == 3 && CHUNKS > 64 && CHUNKS <= 128, "two chunks per lane at most; 64 chunks = 21 rows + 1 chunk");
    const LkOrigin org = lk_tile_origin<W>(jx_max, jy_max, inx, iny);
    const VO_GLOBAL uint8_t *tb = Jimg + (ptrdiff_t)org.y * jstride + org.x;
#ifndef VO_HOST_EMUL
    // the chunk offsets depend on the lane and the level's stride only: seen through, they are hoisted to the level's set-up and
    // live in registers across the iteration loop, which the two-image kernels' bound has no room for
    asm volatile("" : "+v"(lane));
#endif
    const int row = (lane * 43) >> 7, col = lane - CPR * row; // lane / 3, exact below 128
    const uint32_t g0 = (uint32_t)(row * jstride + 16 * col);
    const int next_col = 21 * jstride + 16, next_row = 22 * jstride - 16 * (CPR - 1); // wave-uniform: one select per fill
    const uint32_t g1 = g0 + (uint32_t)(col == CPR - 1 ? next_row : next_col);
    const bool second = lane < CHUNKS - 64;
    const U32x4A4 v0 = *(const VO_GLOBAL U32x4A4 *)(tb + g0);
    U32x4A4 v1 = v0;
    if (second)
        v1 = *(const VO_GLOBAL U32x4A4 *)(tb + g1);
    *reinterpret_cast<uint4 *>(&tile[16 * lane]) = make_uint4(v0.a, v0.b, v0.c, v0.d);
    if (second)
        *reinterpret_cast<uint4 *>(&tile[16 * lane + 1024]) = make_uint4(v1.a, v1.b, v1.c, v1.d);
    return org;
}
// the one-feature kernels: the origin of a tile that covers the window of corner (inx, iny) -- the wave's own if it does, else a
// new one, fetched between two barriers
template <int W = LK_WIN>
__device__ __forceinline__ LkOrigin lk_tile_cover(uint8_t *tile, const VO_GLOBAL uint8_t *__restrict__ Jimg, int jstride, int jx_max, int jy_max,
                                              int inx, int iny, int lane, bool have_tile, int jx0, int jy0)
{
    if (!lk_tile_misses<W>(have_tile, jx0, jy0, inx, iny))
        return LkOrigin{jx0, jy0};
    __syncthreads(); // single-wave workgroup: orders the LDS reads before the refill
    const LkOrigin o = lk_tile_refill_wave<W>(tile, Jimg, jstride, jx_max, jy_max, inx, iny, lane);
    __syncthreads();
    return o;
}
// the pixel pairs of a lane's row segment in the cell at tile offset `off`, upper and lower row: two unaligned 8-byte LDS reads
// (gfx950 handles misaligned ds_read_b64; measured equal to three aligned dwords + v_alignbyte_b32 per row, profiles/r01 notes)
// and the 14 v_perm_b32 of lift7 (the pair kernel, dev/lk_dev.hip) ...
__device__ __forceinline__ void lk_cell_rows(const uint8_t *tile, int off, uint32_t Jt[7], uint32_t Jb[7])
{
    const U32x2A1 t = *reinterpret_cast<const U32x2A1 *>(&tile[off]);
    const U32x2A1 u = *reinterpret_cast<const U32x2A1 *>(&tile[off + LK_JT_W]);
    lift7(t.a, t.b, Jt);
    lift7(u.a, u.b, Jb);
}
// ... or, from the same two reads, the segment's 8 columns as vertical pairs: the 8 v_perm_b32 of lift8_cols (the kernels here)
__device__ __forceinline__ void lk_cell_cols(const uint8_t *tile, int off, uint32_t Jc[8])
{
    const U32x2A1 t = *reinterpret_cast<const U32x2A1 *>(&tile[off]);
    const U32x2A1 u = *reinterpret_cast<const U32x2A1 *>(&tile[off + LK_JT_W]);
    lift8_cols(t.a, t.b, u.a, u.b, Jc);
}

// 7 waves per SIMD = at most 72 VGPRs.  Round 1 had the bound at 6 waves and the allocator happened to land on 70
// registers (so 7 waves were resident anyway); with the round-2 loop it took 78 under that bound -- one wave fewer per
// SIMD, LK 11.9 -> 12.2 ms (gpurun_out/r2_04) -- so the bound now says what is meant: 71 registers, no spills.
// (8 waves = 64 VGPRs spills inside the iteration loop and is slower, gpurun_out/lksweep1.)
#ifndef VO_LK_ATTRS
#define VO_LK_ATTRS __launch_bounds__(64, 7)
#endif
// The body of the kernel.  SPLIT = false: the whole chain (lk_circular_kernel, every batch / lock-step launch).  SPLIT = true
// (lk_hops_kernel, round 6, the synchronous drop-in calls only): hops hop_begin .. hop_end - 1 of the chain -- a launch that does
// not start at hop 0 continues from what the launch before it wrote for hop_begin - 1 (position, status), with the same "this
// feature is going to be dropped anyway" rule, so two launches [0, 1) + [1, 4) write bit for bit what one launch writes.
// ERR = true (lk_flow_kernel): ONE hop, frame = (prev, next) = (Quad::l0, Quad::r0); trk / status are [B][cap], nothing retires
// early, and the level-0 template stays in registers for the err epilogue: err [B][cap] = sum |J(final corner) - I| / (32 * 21 * 21)
// of a point that ends with status 1, else 0 (err == nullptr: not computed).  Everything ERR adds is behind `if constexpr`.
// WIN (lk_flow_win_kernel<W>, with ERR): the window, LkWin<WIN> its lane map.  Everything that depends on the window follows it
// -- halfWin, the +-WIN admissibility tests, the 2 WIN^2 of the min-eigenvalue test, the 32 WIN^2 of err, the tile test and the
// refill's centring -- and what a window below 21 adds (the masks of a row's last segment) is behind `if constexpr` too: for
// WIN = 21 every expression is the constant it was.
// FLAGS (lk_flow_flags_kernel<W>, with ERR): `flags`, wave-uniform, holds the bits of cv::calcOpticalFlowPyrLK's flags --
//   VO_LK_USE_INITIAL_FLOW: at the deepest level the search starts at guess * 2^-level, the guess read from the feature's own
//     output row (trk is in/out: one wave per feature, read at the top, written at the end).  The template side is untouched; a
//     start anywhere goes through the ordinary cell entry (NaN rule, +-WIN admissibility, a first tile centred on the START corner).
//   VO_LK_GET_MIN_EIGENVALS: err = minEig of the level-0 template, the exact expression of the min-eigenvalue test, of every point
//     whose level-0 template window is admissible -- whatever its status ends as -- and 0 of any other; the L1 epilogue and the
//     final in-bounds check that belongs to it do not run, with err == nullptr too (OpenCV: the block is skipped on the flag).
// Everything FLAGS adds is behind `if constexpr`, or -- the test in front of the final check -- a condition that folds to the one it
// was: written any other way, lk_flow_kernel's scalar moves come out in another order (profiles/flow.md, section 6.2).
constexpr int VO_LK_USE_INITIAL_FLOW = 4, VO_LK_GET_MIN_EIGENVALS = 8;
template <bool SPLIT, bool ERR, int WIN = LK_WIN, bool FLAGS = false>
__device__ __forceinline__ void lk_circular_body(const PyrImage *__restrict__ imgs, const Quad *__restrict__ quads,
                                                 const float2 *__restrict__ pts_in, const int *__restrict__ n_pts, int cap,
                                                 int n_frames, int fpg /* 1, 2, 4 or 8 */, int ppp /* features per part */,
                                                 float2 *__restrict__ trk,     // [B][4][cap]
                                                 uint8_t *__restrict__ status, // [B][4][cap]
                                                 const LkParams prm, int hop_begin, int hop_end, float *__restrict__ err = nullptr,
                                                 int flags = 0, int bid = blockIdx.x /* the work item: see below */)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_jt[LK_JT_H * LK_JT_W];

    // XCD-aware block numbering: block id b runs on XCD b % 8 (observed dispatcher behaviour, used
    // for L2 affinity only): XCD x works on frames x, x + 8, x + 16, ... one frame after another.  `bid` is the workgroup's own
    // number in every kernel but lk_circular_queue_kernel, which draws it (vo_lkqueue.h).
    const int xcd = bid & 7, slot = bid >> 3;
    const int grp = slot / ppp, fi = slot - grp * ppp;
    const int frame = grp * fpg + (xcd & (fpg - 1));
    const int f = (xcd / fpg) * ppp + fi;
    if (frame >= n_frames || f >= n_pts[frame])
        return;
    const int lane = threadIdx.x;
    // lane -> (row, 7-pixel segment); lane 63 (WIN = 21; every lane from WIN * SEGS on) duplicates the last live lane's
    // addresses, contributions zeroed
    using LW = LkWin<WIN>;
    const bool live = lane < LW::LANES;
    const int lr = live ? lane : LW::LANES - 1;
    const int r = lr / LW::SEGS, c0 = 7 * (lr - LW::SEGS * r);
    const int lane_off = r * LK_JT_W + c0; // this lane's row segment inside the search tile

    const Quad q = quads[frame];
    const float halfWin = (WIN - 1) * 0.5f;
    const float FLT_SCALE = 1.f / (1 << 20);
    const float eps_lo = (float)(prm.epsilon * 0.999999), eps_hi = (float)(prm.epsilon * 1.000001);
    const float min_eig_n = prm.min_eig * (1.001f * (float)(2 * WIN * WIN)); // see the min-eigenvalue test

    const float2 p = pts_in[(size_t)frame * cap + f];
    float prevPtX = unif(p.x), prevPtY = unif(p.y);
    if (SPLIT && hop_begin > 0) {
        // the chain so far: hop_begin - 1 as the previous launch left it.  A feature that launch saw dead (see the end of the
        // hop loop) has its remaining hops reported already.
        const size_t o = ((size_t)frame * 4 + (hop_begin - 1)) * cap + f;
        const float2 q0 = trk[o];
        const bool dead0 = status[o] == 0 || q0.x < 0.f || q0.y < 0.f || (hop_begin == 1 && (p.x < 0.f || p.y < 0.f));
        if (dead0 && !prm.full_chain)
            return;
        prevPtX = unif(q0.x);
        prevPtY = unif(q0.y);
    }

    for (int hop = SPLIT ? hop_begin : 0; hop < (ERR ? 1 : SPLIT ? hop_end : 4); hop++) {
        // hop chain: l0 -> r0 -> r1 -> l1 -> l0
        const int pi = hop == 0 ? q.l0 : hop == 1 ? q.r0 : hop == 2 ? q.r1 : q.l1;
        const int ni = hop == 0 ? q.r0 : hop == 1 ? q.r1 : hop == 2 ? q.l1 : q.l0;
        const PyrImage &I = imgs[pi];
        const PyrImage &J = imgs[ni];
        // `out` enters the level loop as the point the hop starts from, and every level starts at out * m: m = 2^-level at the
        // deepest level, 2 at every other -- one wave-uniform factor, chosen on the scalar unit, where a select between the scaled
        // start point and 2 * out took two v_cndmask_b32 on the position.  (x * 2.f is x + x bit for bit, NaN and +-inf included.)
        float outX = prm.max_level >= 0 ? prevPtX : 0.f, outY = prm.max_level >= 0 ? prevPtY : 0.f;
        if constexpr (FLAGS) {
            if ((flags & VO_LK_USE_INITIAL_FLOW) && prm.max_level >= 0) { // OpenCV: nextPts[ptidx] * (float)(1. / (1 << level)), one exact multiply
                const float2 g = trk[(size_t)frame * cap + f];
                outX = unif(g.x);
                outY = unif(g.y);
            }
        }
        int st = 1;
        float errv = 0.f; // (ERR)

        for (int level = prm.max_level; level >= 0; level--) {
            const float scale = __int_as_float((127 - level) << 23); // 2^-level, exact (no divide)
            float prevX = prevPtX * scale, prevY = prevPtY * scale;
            // (chosen as an integer: a wave-uniform select between floats is a v_cndmask_b32, between integers an s_cselect_b32)
            const float start = __int_as_float(level == prm.max_level ? (127 - level) << 23 : 0x40000000);
            outX *= start;
            outY *= start;
            float nextX = outX, nextY = outY;

            const int iw = I.w[level], ih = I.h[level], istride = I.stride[level];
            const int jw = J.w[level], jh = J.h[level], jstride = J.stride[level];
            const VO_GLOBAL uint8_t *__restrict__ Iimg = (const VO_GLOBAL uint8_t *)I.lvl[level];
            const VO_GLOBAL uint32_t *__restrict__ Ider = (const VO_GLOBAL uint32_t *)I.der[level];
            const VO_GLOBAL uint8_t *__restrict__ Jimg = (const VO_GLOBAL uint8_t *)J.lvl[level];

            prevX -= halfWin;
            prevY -= halfWin;
            const float fpx = floorf(prevX), fpy = floorf(prevY);
            const int ipx = uni(cvt_i32_f32(fpx)), ipy = uni(cvt_i32_f32(fpy));
            // x86's cvFloor(NaN) is INT_MIN (cvttss2si), i.e. "left of the window": OpenCV rejects a NaN coordinate here.
            // v_cvt_i32_f32(NaN) is 0, which would ADMIT it -- so NaN is rejected on the float (one
            // v_cmp_u_f32 into a scalar pair).  +-inf and finite values beyond int32 saturate to the rejected side on both.
            if (VO_BALLOT(__builtin_isunordered(fpx, fpy)) != 0ull || ipx < -WIN || ipx >= iw || ipy < -WIN || ipy >= ih) {
                if (level == 0)
                    st = 0;
                continue;
            }
            uint32_t wl, wr; // (float)ipx == floorf(prevX): the fractional part needs no int round trip
            lk_weights_cols(prevX - fpx, prevY - fpy, wl, wr);

            // ---- 21 x 21 template straight from the bordered pyramid (registers) + structure tensor --
            // lane: pixels (ipx + c0 .. + 7, ipy + r) and the row below; the bordered layout makes
            // every admissible window an in-bounds read (reflected pixels, zero derivatives)
            // b1 = sum (J - I) * Ix is accumulated as sum J * Ix - sum I * Ix: the lane's own (exact, integer)
            // sum I * Ix is formed once per level and seeds the iteration's accumulator, so the inner loop
            // neither keeps I nor subtracts it
            uint32_t Ixp[4], Iyp[4];
            uint32_t Ipe[ERR ? 4 : 1]; // (ERR) the template's pixels, kept for the err epilogue
            int a11 = 0, a12 = 0, a22 = 0, c1 = 0, c2 = 0;
            {
                // Addresses as a wave-uniform base (first element of the bordered allocation, scalar registers) plus a
                // per-lane 32-bit offset that is never negative: what global_load's scalar-base form takes, instead
                // of 64-bit per-lane pointer arithmetic.
                const ptrdiff_t org = (ptrdiff_t)VO_BY * istride + VO_BX;
                const VO_GLOBAL uint8_t *Ib = Iimg - org;
                const VO_GLOBAL uint8_t *Db = (const VO_GLOBAL uint8_t *)(Ider - org); // byte offsets: 4 * od fits 32 bits
                const uint32_t o = (uint32_t)((ipy + r + VO_BY) * istride + ipx + c0 + VO_BX);
                // lane 63 owns no pixel: it reads its Scharr samples from the (all-zero) top-left border
                // corner, so Ix = Iy = 0 there and every sum it feeds is 0 without any select
                const uint32_t od = live ? 4u * o : 0u, drow = 4u * (uint32_t)istride;
                const U32x2A1 t = *(const VO_GLOBAL U32x2A1 *)(Ib + o);
                const U32x2A1 u = *(const VO_GLOBAL U32x2A1 *)(Ib + (o + (uint32_t)istride));
                const U32x4A4 dt0 = *(const VO_GLOBAL U32x4A4 *)(Db + od);
                const U32x4A4 dt1 = *(const VO_GLOBAL U32x4A4 *)(Db + (od + 16u));
                const U32x4A4 db0 = *(const VO_GLOBAL U32x4A4 *)(Db + (od + drow));
                const U32x4A4 db1 = *(const VO_GLOBAL U32x4A4 *)(Db + (od + drow + 16u));
                const uint32_t dt[8] = {dt0.a, dt0.b, dt0.c, dt0.d, dt1.a, dt1.b, dt1.c, dt1.d};
                const uint32_t db[8] = {db0.a, db0.b, db0.c, db0.d, db1.a, db1.b, db1.c, db1.d};
                uint32_t Ip[4];
                bilinear7_u8_cols(t.a, t.b, u.a, u.b, wl, wr, Ip);
                bilinear7_deriv_cols(dt, db, wl, wr, Ixp, Iyp);
                if constexpr (LW::LAST < 7) {
                    // the last segment of a row reaches beyond the window: its pixels from LAST on get Ix = Iy = 0, once per
                    // level, so that A11 / A12 / A22, the seeds c1 / c2 and every b1 / b2 of the iteration take nothing from them
                    const bool part = LW::SEGS == 1 || c0 == 7 * (LW::SEGS - 1);
#pragma unroll
                    for (int m = 0; m < 4; m++) {
                        const uint32_t keep = part ? lk_seg_mask(LW::LAST, m) : 0xffffffffu;
                        Ixp[m] &= keep;
                        Iyp[m] &= keep;
                    }
                }
                a11 = sdot2_first(Ixp[0], Ixp[0], 0);
                a12 = sdot2_first(Ixp[0], Iyp[0], 0);
                a22 = sdot2_first(Iyp[0], Iyp[0], 0);
                c1 = sdot2_first(Ip[0], Ixp[0], 0);
                c2 = sdot2_first(Ip[0], Iyp[0], 0);
#pragma unroll
                for (int m = 1; m < 4; m++) {
                    a11 = sdot2(Ixp[m], Ixp[m], a11);
                    a12 = sdot2(Ixp[m], Iyp[m], a12);
                    a22 = sdot2(Iyp[m], Iyp[m], a22);
                    c1 = sdot2(Ip[m], Ixp[m], c1);
                    c2 = sdot2(Ip[m], Iyp[m], c2);
                }
                if constexpr (ERR) {
#pragma unroll
                    for (int m = 0; m < 4; m++)
                        Ipe[m] = Ip[m];
                }
            }
            float A11, A12, A22;
            wave_sum3_exact_f32(a11, a12, a22, A11, A12, A22);
            // can b1, b2 of this level's iterations exceed 32 bits (vo_lkmath.h)?  Wave-uniform, from the two sums as they come out
            // of v_readlane -- scalar registers --, before the 2^-20
            const bool fit = lk_sums_fit(A11, A22);
            A11 *= FLT_SCALE;
            A12 *= FLT_SCALE;
            A22 *= FLT_SCALE;

            float D = A11 * A22 - A12 * A12;
            // OpenCV: minEig = (A22 + A11 - sqrt((A11-A22)^2 + 4 A12^2)) / (2 * 21 * 21), rejected when < minEigThreshold
            // (882 = 2 * 21 * 21 below stands for 2 * WIN * WIN: the argument holds for any positive constant).
            // The correctly rounded sqrt and divide cost ~30 wave-uniform VALU instructions, and the test is almost
            // never close: with t = A22 + A11, s2 = the radicand and u = t - (1.001 * 882 * thr + t * 2^-18),
            // "u > 0 and s2 < 0.9999 u^2" implies sqrt(s2) < u (1 - 4e-5), hence the rounded t - sqrt(s2) exceeds
            // 1.0009 * 882 * thr and the rounded quotient exceeds thr (every rounding involved is below 2^-23
            // relative, the margins are 1e-3 and 2^-18 t): the exact expression cannot reject.  Otherwise evaluate it.
            const float t = A22 + A11;
            const float s2 = (A11 - A22) * (A11 - A22) + 4.f * A12 * A12;
            const float u = t - (min_eig_n + t * 3.814697265625e-6f);
            bool eig_ok = u > 0.f && s2 < u * u * 0.9999f;
            if (__builtin_expect(!eig_ok, 0)) {
#ifndef VO_HOST_EMUL
                asm volatile("" ::: "memory"); // keep the sqrt / divide out of the common path
#endif
                const float minEig = (t - sqrtf(s2)) / (float)(2 * WIN * WIN);
                eig_ok = !(minEig < prm.min_eig);
            }
            if constexpr (FLAGS) {
                // (the shortcut above still decides; the value itself is wanted once per feature, admitted or not)
                if ((flags & VO_LK_GET_MIN_EIGENVALS) && level == 0)
                    errv = (t - sqrtf(s2)) / (float)(2 * WIN * WIN);
            }
            if (!eig_ok || D < FLT_EPSILON) {
                if (level == 0)
                    st = 0;
                continue;
            }
            D = rcp_normal_f32(D); // FLT_EPSILON <= D < 2^29 (vo_isa.h)
            // b1, b2 carry the same 2^-20 as the A's; a power of two moves through the rounded products unchanged
            // (A12 * (S * 2^-20) == (A12 * 2^-20) * S bit for bit), so it is folded into the A's once per level
            const float A11s = A11 * FLT_SCALE, A12s = A12 * FLT_SCALE, A22s = A22 * FLT_SCALE;
            const int nc1 = -c1, nc2 = -c2;

            nextX -= halfWin;
            nextY -= halfWin;
            int jx0 = 0, jy0 = 0;
            bool have_tile = false;
            // tile origins that keep the 40 x 48 tile inside the level's rectangle (vo_dev.h, "reads stay inside their level"):
            // the last tile ends exactly at the row end (column jstride - VO_BX - 1) and at the last border row
            static_assert(LK_JT_W % 16 == 0 && VO_BX % 4 == 0, "16-byte tile chunks at 4-byte aligned origins");
            // (the right border of a row is stride - VO_BX - w >= VO_BY columns -- level_stride pads the row by VO_BY and rounds up --
            // so VO_BY is the column border the reads of a corner at w - 1 rely on, as it is the row border below h - 1)
            static_assert(VO_BY >= WIN && LK_JT_W >= LW::COLS + LW::OFF_X + 3 && LK_JT_H >= LW::ROWS + LW::OFF_Y,
                          "a tile clamped to the row end / the last border row still covers what the window of every corner the "
                          "reference admits reads (up to w - 1, h - 1: the borders are at least a window wide)");
            static_assert(VO_BY >= LW::COLS - 1, "right border (at least VO_BY columns) >= the columns a row reads beyond corner w - 1");
            const int jx_max = jstride - VO_BX - LK_JT_W, jy_max = jh + VO_BY - LK_JT_H;

            // The window corner stays in the same pixel cell for two iterations out of three, so everything that only depends on
            // the cell -- tile test / refill, LDS address, the two row reads and the 8 v_perm_b32 that lift the segment's columns
            // into registers -- sits behind a wave-uniform "another cell" branch at the top of ONE loop: position, floors, deltas
            // and the iteration count live in one set of registers, where an outer loop per cell and an inner loop per iteration
            // copied them at every cell entry and back.  The admissibility test of a new cell sits where the cell is left (and
            // in front of the loop for the first one), so the block behind the branch has no way out of the loop.
            int j = 0;
            // how the loop was left: 0 = before any iteration of this level (out stays the level's start value: (x - halfWin) +
            // halfWin is not x), else behind an iteration (out = next + halfWin): 1 = epsilon or count, 2 / 3 = the oscillation test,
            // the delta of the half step back in (dAx, dAy) / (dBx, dBy), 4 = the next cell is not admitted
            int left = 0;
            // floors and fractions of the corner: set by cell_admitted / enter_cell before anything reads them, by nothing before
            // that (like the columns below: no moves per level to zero what the first cell overwrites)
            float fnx, fny, frx, fry;
#ifndef VO_HOST_EMUL
            asm volatile("" : "=v"(fnx), "=v"(fny));
#else
            fnx = fny = frx = fry = 0.f;
#endif
            // the cell's columns (two window rows per lane) as vertical pixel pairs: eight scalars, not an array -- an array carried
            // round the loop becomes one 8-register tuple, copied at every cell entry -- and set by nothing before the first cell
            // (the device's "set by nothing" stands at the top of each version of the loop, below)
            uint32_t J0, J1, J2, J3, J4, J5, J6, J7;
#ifdef VO_HOST_EMUL
            J0 = J1 = J2 = J3 = J4 = J5 = J6 = J7 = 0;
#endif
            int inx = 0, iny = 0;
            bool cell = true; // the corner is in another pixel cell than the registers hold (wave-uniform)
            // the cell of the corner, and whether the reference admits it.  x86's cvFloor(NaN) is INT_MIN: rejected (see the template)
            auto cell_admitted = [&]() -> bool {
                fnx = floorf(nextX);
                fny = floorf(nextY);
                inx = uni(cvt_i32_f32(fnx));
                iny = uni(cvt_i32_f32(fny));
                return !(VO_BALLOT(__builtin_isunordered(fnx, fny)) != 0ull || inx < -WIN || inx >= jw || iny < -WIN || iny >= jh);
            };
            auto enter_cell = [&]() {
                {
                    const LkOrigin o = lk_tile_cover<WIN>(s_jt, Jimg, jstride, jx_max, jy_max, inx, iny, lane, have_tile, jx0, jy0);
                    jx0 = o.x;
                    jy0 = o.y;
                    have_tile = true;
                }
                uint32_t Jn[8];
                lk_cell_cols(s_jt, (iny - jy0) * LK_JT_W + (inx - jx0) + lane_off, Jn); // uniform part on the scalar unit
                J0 = Jn[0], J1 = Jn[1], J2 = Jn[2], J3 = Jn[3], J4 = Jn[4], J5 = Jn[5], J6 = Jn[6], J7 = Jn[7];
                frx = nextX - fnx;
                fry = nextY - fny;
            };
            // One iteration: the delta into (dx, dy), tested against the one before it in (px, py).  Returns 0 = go on, or how the
            // loop is left (a value, not a write to `left` / `st` from in here: behind the barriers below those would live in memory).
            // (frx, fry) = the fractional position of the window corner inside its pixel cell: the bilinear weights come from it,
            // and the corner is still inside the cell exactly as long as both parts are in [0, 1).  fl(nextX - fnx) is what
            // OpenCV itself computes (nextPt.x - inextPt.x); a true difference >= 1 or < 0 can never round into [0, 1),
            // so "inside" is never wrong -- a spurious "left" (difference just below 1 rounding up to 1.0) only
            // re-enters the same cell.  As raw bits, [0, 1) is "below 0x3f800000, unsigned" (negative values have the
            // sign bit set), so one unsigned max + one compare replace two floors, two compares and two selects per
            // iteration; the two differences of that test are the next iteration's weight inputs.
            // `fitc` (std::true_type / std::false_type): the level's word on its sums, as a type -- the loop below exists once per value
            auto iterate = [&](auto fitc, const float px, const float py, float &dx, float &dy, const int osc) -> int {
                constexpr bool FIT = decltype(fitc)::value;
                lk_weights_cols(frx, fry, wl, wr);
                int b1, b2;
                {
                    const uint32_t Jc[8] = {J0, J1, J2, J3, J4, J5, J6, J7};
                    uint32_t Jp[4];
                    // iw11 = -1 (the sign of wr, the same in every lane) through a scalar: a branch of the wave, not a region
                    // that rewrites the execution mask around a case that almost never occurs
                    const bool neg = uni((int)wr) < 0;
                    VO_LK_COUNT_NEG(neg);
                    blend7_cols(Jc, wl, wr, neg, Jp);
                    b1 = sdot2_first(Jp[0], Ixp[0], nc1); // seeds: minus the lane's sum I * Ix, sum I * Iy
                    b2 = sdot2_first(Jp[0], Iyp[0], nc2);
#pragma unroll
                    for (int m = 1; m < 4; m++) {
                        b1 = sdot2(Jp[m], Ixp[m], b1);
                        b2 = sdot2(Jp[m], Iyp[m], b2);
                    }
                }
                float fb1, fb2;
                VO_LK_COUNT_FIT(level, FIT);
                wave_sum2_f32<FIT>(b1, b2, fb1, fb2); // (10 VALU instructions where the sums fit, else 15)
                dx = (A12s * fb2 - A22s * fb1) * D;
                dy = (A12s * fb1 - A11s * fb2) * D;
                nextX += dx;
                nextY += dy;
                // OpenCV: delta.ddot(delta) <= epsilon in f64.  The f32 value n2 is within 2^-23 of it, so it
                // decides on its own unless it falls inside a 1e-6 band around epsilon (then the f64 form).  The hot
                // path carries ONE compare ("clearly not converged"); everything else happens once per level.
                const float n2 = fmaf(dy, dy, dx * dx);
                if (__builtin_expect(!(n2 > eps_hi), 0)) {
#ifndef VO_HOST_EMUL
                    asm volatile("" ::: "memory"); // keep the rare evaluation out of the hot path
#endif
                    if (n2 < eps_lo || (double)dx * dx + (double)dy * dy <= prm.epsilon)
                        return 1;
                }
                // OpenCV: std::abs(delta.x + prevDelta.x) < 0.01 (f32 sum compared as double).  0.01f is
                // the largest f32 below the double 0.01, so for an f32 s:  |s| < 0.01  <=>  |s| <= 0.01f
                if (j > 0 && fabsf(dx + px) <= 0.01f && fabsf(dy + py) <= 0.01f)
                    return osc;
                if (++j >= prm.max_count)
                    return 1;
                frx = nextX - fnx;
                fry = nextY - fny;
                const uint32_t ua = (uint32_t)__float_as_int(frx), ub = (uint32_t)__float_as_int(fry);
                cell = VO_BALLOT((ua > ub ? ua : ub) >= 0x3f800000u) != 0ull; // the corner left the cell
                if (cell && !cell_admitted())
                    return 4;
                return 0;
            };
            // the previous delta is the other half's delta: unrolled by two with the roles of the two pairs exchanged, no copy
            float dAx = 0.f, dAy = 0.f, dBx = 0.f, dBy = 0.f;
            bool run = prm.max_count > 0;
            if (run && !cell_admitted()) {
                if (level == 0)
                    st = 0;
                run = false;
            }
            // The loop, once for each kind of sum and chosen once per level: `fit` is the same for every iteration of the level, and
            // as a value tested inside the iteration it cost two scalar branches and a mask in a scalar pair in each of them
            // (profiles/r12_lk_iteration_branches.md).  Returns how the loop was left.
            auto solve = [&](auto fitc) -> int {
                // The region is compiled with a path from the first loop into the second, so what enters the second loop lives
                // through the first.  The corner and its floors would: four registers the chain kernels do not have.  They are formed
                // again per version instead, from `out`, which the loops leave alone -- the same operations on the same values as in
                // front of the loop, with the constant through a scalar the compiler does not see through, or it takes the results
                // it has.  (A scalar: an opaque vector register counts as a value per lane, and `st` and the hop's start point, which
                // depend on the corner, then move from scalar registers into vector ones.)
                int hw = __float_as_int(halfWin);
#ifndef VO_HOST_EMUL
                asm volatile("" : "+s"(hw));
                // what the first cell overwrites, undefined per version: defined once in front of both, the two loops get a set of
                // registers each and a copy of every one at their entry
                asm volatile("" : "=v"(frx), "=v"(fry));
                asm volatile("" : "=v"(J0), "=v"(J1), "=v"(J2), "=v"(J3), "=v"(J4), "=v"(J5), "=v"(J6), "=v"(J7));
#endif
                nextX = outX - __int_as_float(hw);
                nextY = outY - __int_as_float(hw);
                fnx = floorf(nextX);
                fny = floorf(nextY);
                for (;;) {
                    if (cell)
                        enter_cell();
                    if (const int l = iterate(fitc, dBx, dBy, dAx, dAy, 2))
                        return l;
                    if (cell)
                        enter_cell();
                    if (const int l = iterate(fitc, dAx, dAy, dBx, dBy, 3))
                        return l;
                }
            };
            if (run)
                left = fit ? solve(std::true_type{}) : solve(std::false_type{});
            if (left == 4 && level == 0) // the corner left the image behind an iteration
                st = 0;
            // out = next + halfWin, read only here; the rounding order of the half step is (next + halfWin) - d * 0.5
            if (left != 0) {
#ifndef VO_HOST_EMUL
                asm volatile("" ::: "memory"); // a branch, not selects on a copy of `left` made in every iteration
#endif
                outX = nextX + halfWin;
                outY = nextY + halfWin;
                if (left == 2 || left == 3) {
#ifndef VO_HOST_EMUL
                    asm volatile("" ::: "memory");
#endif
                    outX -= (left == 2 ? dAx : dBx) * 0.5f;
                    outY -= (left == 2 ? dAy : dBy) * 0.5f;
                }
            }

            // final in-bounds check OpenCV performs at level 0 when an err vector is requested
            // (st == 1 here means the last cell entry was admitted and every delta since was finite: outX / outY are finite,
            // possibly huge -- both conversions then land on a rejected side, x86's INT_MIN and gfx950's saturated INT_MAX)
            // ((FLAGS) not in the min-eigenvalue mode: OpenCV skips the whole block on that flag)
            if (st && level == 0 && (!FLAGS || !(flags & VO_LK_GET_MIN_EIGENVALS))) {
                const int fx = vo_f2i(floorf(outX - halfWin)), fy = vo_f2i(floorf(outY - halfWin));
                if (fx < -WIN || fx >= jw || fy < -WIN || fy >= jh)
                    st = 0;
                if constexpr (ERR) {
                    // err of cv::calcOpticalFlowPyrLK (lkpyramid.cpp, the block behind the iterations): the window at the corner of
                    // the FINAL position (after a possible half step back: another cell, possibly outside the tile) against the
                    // template, sum |Jp - Ip| over the 441 pixels / (32 * 21 * 21).  The integer sum is below 441 * 8160 < 2^24, so
                    // rounding it once is the reference's running f32 sum bit for bit (WIN * WIN <= 441 pixels; those a row's last
                    // segment holds beyond the window are masked like their derivatives).
                    if (st && err != nullptr) {
                        const float ex = outX - halfWin, ey = outY - halfWin;
                        const float fex = floorf(ex), fey = floorf(ey);
                        const int inx = uni(fx), iny = uni(fy); // (admitted just above: inside [-21, jw) x [-21, jh))
                        const LkOrigin o = lk_tile_cover<WIN>(s_jt, Jimg, jstride, jx_max, jy_max, inx, iny, lane, have_tile, jx0, jy0);
                        jx0 = o.x;
                        jy0 = o.y;
                        uint32_t Jc[8], Jp[4];
                        lk_cell_cols(s_jt, (iny - jy0) * LK_JT_W + (inx - jx0) + lane_off, Jc);
                        lk_weights_cols(ex - fex, ey - fey, wl, wr);
                        blend7_cols(Jc, wl, wr, Jp);
                        uint32_t e = 0; // lane 63 duplicates lane 62's pixels: it contributes nothing
#pragma unroll
                        for (int m = 0; m < 4; m++) {
                            // (the unmasked case keeps the statement it always was: with one shape for both, lk_flow_kernel's
                            // instruction stream comes out with two scalar moves exchanged)
                            if constexpr (LW::LAST < 7) {
                                const bool part = LW::SEGS == 1 || c0 == 7 * (LW::SEGS - 1);
                                e = udot2(pk_absdiff_i16(Jp[m], Ipe[m]) & (part ? lk_seg_mask(LW::LAST, m) : 0xffffffffu), 0x00010001u, e);
                            } else
                                e = udot2(pk_absdiff_i16(Jp[m], Ipe[m]), 0x00010001u, e);
                        }
                        errv = wave_sum_exact_f32(live ? (int)e : 0) / (float)(32 * WIN * WIN);
                    }
                }
            }
        }

        if constexpr (ERR) {
            if (lane == 0) {
                trk[(size_t)frame * cap + f] = make_float2(outX, outY);
                status[(size_t)frame * cap + f] = (uint8_t)st;
                if (err != nullptr) {
                    if constexpr (FLAGS) // (errv of the min-eigenvalue mode is 0 unless the level-0 template was admitted)
                        err[(size_t)frame * cap + f] = ((flags & VO_LK_GET_MIN_EIGENVALS) || st) ? errv : 0.f;
                    else
                        err[(size_t)frame * cap + f] = st ? errv : 0.f;
                }
            }
            return;
        }
        if (lane == 0) {
            trk[((size_t)frame * 4 + hop) * cap + f] = make_float2(outX, outY);
            status[((size_t)frame * 4 + hop) * cap + f] = (uint8_t)st;
        }
        // deleteUnmatchFeaturesCircle (feature.cpp:96-104) drops the feature if any hop failed or any
        // of pt0..pt3 has a negative coordinate: nothing computed after that point can reach an output
        // of circularMatching(), so the wave retires (remaining hops reported as status 0)
        const bool dead = st == 0 || outX < 0.f || outY < 0.f || (hop == 0 && (p.x < 0.f || p.y < 0.f));
        if (dead && !prm.full_chain && hop < 3) {
            if (lane == 0)
                for (int k = hop + 1; k < 4; k++) {
                    trk[((size_t)frame * 4 + k) * cap + f] = make_float2(-1.f, -1.f);
                    status[((size_t)frame * 4 + k) * cap + f] = 0;
                }
            return;
        }
        prevPtX = unif(outX);
        prevPtY = unif(outY);
    }
}

__global__ VO_LK_ATTRS void lk_circular_kernel(const PyrImage *__restrict__ imgs,
                                                          const Quad *__restrict__ quads,
                                                          const float2 *__restrict__ pts_in,
                                                          const int *__restrict__ n_pts, int cap,
                                                          int n_frames, int fpg /* 1, 2, 4 or 8 */,
                                                          int ppp /* features per part */,
                                                          float2 *__restrict__ trk,      // [B][4][cap]
                                                          uint8_t *__restrict__ status,  // [B][4][cap]
                                                          LkParams prm)
{
    lk_circular_body<false, false>(imgs, quads, pts_in, n_pts, cap, n_frames, fpg, ppp, trk, status, prm, 0, 4);
}

// The same chain with the work item drawn from the per-XCD ticket queues of vo_lkqueue.h (batches of LKQ_MIN_FRAMES frames and
// more): lane 0 takes a ticket of its XCD's queue -- relaxed, agent scope: the queues are shared by the eight XCDs, so the
// counter must not live in one XCD's L2 --, the wave gets it through a scalar, and a wave that finds its queue dry takes from the
// next one; the wave that finds all eight dry marks its XCD's counter, and the XCD's later waves end at their first draw.
// `next`: this launch's eight counters, LKQ_STRIDE words apart; `other`: the set of the launch before, which nothing reads any
// more (launches on the tracking stream do not overlap) and block 0 zeroes for the launch after this one.  Results are those of
// lk_circular_kernel bit for bit: only which workgroup computes a feature changes.
__device__ __forceinline__ unsigned lk_queue_draw(unsigned *next, int q)
{
#ifdef VO_HOST_EMUL // (lanes run one at a time between yields: the plain read-modify-write is atomic)
    unsigned t = 0;
    if (threadIdx.x == 0)
        t = next[LKQ_STRIDE * q]++;
#else
    unsigned t = 0;
    if (threadIdx.x == 0)
        t = __hip_atomic_fetch_add(&next[LKQ_STRIDE * q], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
    return (unsigned)uni((int)t);
}
// lk_queue_take's mark, in the shape of the draw: lane 0's atomic, its result through a scalar and dropped.  Nothing needs the
// result; written as an atomic nobody waits for, the allocator ends at 72 registers and 23 spilled ones, where in
// this shape the kernel keeps lk_circular_kernel's 64 (profiles/r10_lk_xcd_queue.md, section 4).  One workgroup per XCD and
// launch comes here, or the few that find the queues dry at the same time.
__device__ __forceinline__ void lk_queue_mark(unsigned *next, int q)
{
    unsigned t = 0;
#ifdef VO_HOST_EMUL
    if (threadIdx.x == 0)
        next[LKQ_STRIDE * q] |= LKQ_ALL_DRY;
    (void)uni((int)t);
#else
    if (threadIdx.x == 0)
        t = __hip_atomic_fetch_or(&next[LKQ_STRIDE * q], LKQ_ALL_DRY, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("" ::"s"(uni((int)t)));
#endif
}
__global__ VO_LK_ATTRS void lk_circular_queue_kernel(const PyrImage *__restrict__ imgs, const Quad *__restrict__ quads,
                                                     const float2 *__restrict__ pts_in, const int *__restrict__ n_pts, int cap,
                                                     int n_frames, int fpg /* 8 */, int ppp, float2 *__restrict__ trk,
                                                     uint8_t *__restrict__ status, LkParams prm, int items /* per queue */,
                                                     unsigned *next, unsigned *other)
{
    if (blockIdx.x == 0 && threadIdx.x < (unsigned)LKQ_QUEUES) {
#ifdef VO_HOST_EMUL
        other[LKQ_STRIDE * threadIdx.x] = 0u;
#else
        __hip_atomic_store(&other[LKQ_STRIDE * threadIdx.x], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
    }
    const int bid = lk_queue_take((int)(blockIdx.x & 7), items, [&](int q) { return lk_queue_draw(next, q); },
                                  [&](int q) { lk_queue_mark(next, q); });
    if (bid < 0)
        return;
    lk_circular_body<false, false>(imgs, quads, pts_in, n_pts, cap, n_frames, fpg, ppp, trk, status, prm, 0, 4, nullptr, 0, bid);
}

// Hops hop_begin .. hop_end - 1 only: the synchronous drop-in calls (capi_run.hip) launch hop 0 -- which reads the t0 pair
// only -- while the t1 pair is still crossing PCIe and its pyramids are being built on another stream, then hops 1 .. 3.
__global__ VO_LK_ATTRS void lk_hops_kernel(const PyrImage *__restrict__ imgs, const Quad *__restrict__ quads,
                                           const float2 *__restrict__ pts_in, const int *__restrict__ n_pts, int cap,
                                           int n_frames, int fpg, int ppp, float2 *__restrict__ trk,
                                           uint8_t *__restrict__ status, LkParams prm, int hop_begin, int hop_end)
{
    lk_circular_body<true, false>(imgs, quads, pts_in, n_pts, cap, n_frames, fpg, ppp, trk, status, prm, hop_begin, hop_end);
}

// One hop between the images (Quad::l0 -> Quad::r0) of every frame with the err output (see lk_circular_body, ERR).  The err
// epilogue needs the template's four registers beyond the iteration loop and a second blend: under the product kernels' bound of
// 71 registers the allocator spills inside the loop, so this kernel takes 6 waves per SIMD (profiles/flow.md).
#ifndef VO_LK_FLOW_ATTRS
#define VO_LK_FLOW_ATTRS __launch_bounds__(64, 6)
#endif
__global__ VO_LK_FLOW_ATTRS void lk_flow_kernel(const PyrImage *__restrict__ imgs, const Quad *__restrict__ pairs,
                                                const float2 *__restrict__ pts_in, const int *__restrict__ n_pts, int cap,
                                                int n_frames, int fpg, int ppp, float2 *__restrict__ next, // [B][cap]
                                                uint8_t *__restrict__ status,                               // [B][cap]
                                                float *__restrict__ err /* [B][cap] or null */, LkParams prm)
{
    lk_circular_body<false, true>(imgs, pairs, pts_in, n_pts, cap, n_frames, fpg, ppp, next, status, prm, 0, 1, err);
}

// The same hop with a W x W window, W odd in 5 .. 19 (vowin_*, capi_flow.hip; W = 21 is lk_flow_kernel): the body with
// WIN = W, one instantiation per window.  Register reports of the eight: profiles/flow.md.
template <int W>
__global__ VO_LK_FLOW_ATTRS void lk_flow_win_kernel(const PyrImage *__restrict__ imgs, const Quad *__restrict__ pairs,
                                                    const float2 *__restrict__ pts_in, const int *__restrict__ n_pts, int cap,
                                                    int n_frames, int fpg, int ppp, float2 *__restrict__ next, // [B][cap]
                                                    uint8_t *__restrict__ status,                               // [B][cap]
                                                    float *__restrict__ err /* [B][cap] or null */, LkParams prm)
{
    static_assert(W < LK_WIN, "21 is lk_flow_kernel");
    lk_circular_body<false, true, W>(imgs, pairs, pts_in, n_pts, cap, n_frames, fpg, ppp, next, status, prm, 0, 1, err);
}

// The same hop with cv::calcOpticalFlowPyrLK's flags (voflag_*, include/vo_flow_flags.h): the body with FLAGS, one instantiation
// per odd W of 5 .. 21 -- 21 included: lk_flow_kernel stays what it is -- and the two flag bits as a wave-uniform argument, not as
// template parameters (27 more copies of this body).  `next` is in/out.  Register reports of the nine: profiles/flow.md.
template <int W>
__global__ VO_LK_FLOW_ATTRS void lk_flow_flags_kernel(const PyrImage *__restrict__ imgs, const Quad *__restrict__ pairs,
                                                      const float2 *__restrict__ pts_in, const int *__restrict__ n_pts, int cap,
                                                      int n_frames, int fpg, int ppp, float2 *__restrict__ next, // [B][cap], in/out
                                                      uint8_t *__restrict__ status,                               // [B][cap]
                                                      float *__restrict__ err /* [B][cap] or null */, LkParams prm, int flags)
{
    lk_circular_body<false, true, W, true>(imgs, pairs, pts_in, n_pts, cap, n_frames, fpg, ppp, next, status, prm, 0, 1, err, flags);
}

// The launch geometry of the block numbering above: frames per group of 8 XCDs (the largest power of two <= min(8, n_frames)),
// work items -- features, or the pair kernel's pairs of features (dev/lk_dev.hip) -- per part of a frame's list, and the number
// of workgroups.  Host code; the CPU emulator of the tests launches by it too.
struct LkGrid {
    int fpg, ppp, blocks;
};
inline LkGrid lk_grid(int n_frames, int n_items)
{
    const int fpg = n_frames >= 8 ? 8 : n_frames >= 4 ? 4 : n_frames >= 2 ? 2 : 1;
    const int parts = 8 / fpg, ppp = (n_items + parts - 1) / parts;
    const int groups = (n_frames + fpg - 1) / fpg;
    return {fpg, ppp, 8 * groups * ppp};
}

// The windows of the two-image kernels, listed once: f(std::integral_constant<int, W>) for the odd W of 5 .. 21 that `win` is;
// false, and f not called, for any other window.
template <int... W, typename F>
inline bool lk_visit_window(int win, F &&f)
{
    return ((win == W && (f(std::integral_constant<int, W>{}), true)) || ...);
}
template <typename F>
inline bool lk_for_window(int win, F &&f)
{
    return lk_visit_window<5, 7, 9, 11, 13, 15, 17, 19, LK_WIN>(win, f);
}

// The route from (W, flags) to a two-image kernel, written once: run(kernel, arguments behind prm...).  Flags are
// lk_flow_flags_kernel<W>, which takes them as its last argument; without, 21 is lk_flow_kernel and any other W its own kernel.
template <int W, typename R>
inline void lk_flow_route(int flags, R &&run)
{
    if (flags != 0)
        run(lk_flow_flags_kernel<W>, flags);
    else if constexpr (W == LK_WIN)
        run(lk_flow_kernel);
    else
        run(lk_flow_win_kernel<W>);
}

#ifndef VO_HOST_EMUL
// (vo_kernels.h has the preconditions; the entry points of capi_flow.hip refuse what breaks them before anything else happens)
void launch_lk_flow(int win, int flags, const PyrImage *d_imgs, const Quad *d_pairs, const float2 *d_pts, const int *d_npts, int cap,
                    int max_pts, int n_frames, float2 *d_next, uint8_t *d_status, float *d_err, const LkParams &prm, hipStream_t stream)
{
    if (max_pts <= 0 || n_frames <= 0 || (flags & ~(VO_LK_USE_INITIAL_FLOW | VO_LK_GET_MIN_EIGENVALS)))
        return;
    const LkGrid g = lk_grid(n_frames, max_pts);
    lk_for_window(win, [&](auto w) {
        lk_flow_route<decltype(w)::value>(flags, [&](auto kernel, auto... tail) {
            hipLaunchKernelGGL(kernel, dim3((unsigned)g.blocks), dim3(64), 0, stream, d_imgs, d_pairs, d_pts, d_npts, cap, n_frames, g.fpg,
                               g.ppp, d_next, d_status, d_err, prm, tail...);
        });
    });
}

void launch_lk_circular(const PyrImage *d_imgs, const Quad *d_quads, const float2 *d_pts, const int *d_npts,
                        int cap, int max_pts, int n_frames, float2 *d_trk, uint8_t *d_status,
                        const LkParams &prm, hipStream_t stream, LkQueues *queues)
{
    if (max_pts <= 0 || n_frames <= 0)
        return;
    // batches of 16 frames and more: the work items from the per-XCD queues (a context without counters, or a launch whose
    // ticket range would not fit an int, keeps the static split)
    if (queues != nullptr && queues->d_next != nullptr && n_frames >= LKQ_MIN_FRAMES &&
        (long long)((n_frames + 7) / 8) * max_pts < (1ll << 26)) {
        const LkQueueGrid g = lk_queue_grid(n_frames, max_pts);
        const int set = queues->launches++ & 1;
        unsigned *const cur = queues->d_next + set * (LKQ_QUEUES * LKQ_STRIDE);
        unsigned *const oth = queues->d_next + (set ^ 1) * (LKQ_QUEUES * LKQ_STRIDE);
        hipLaunchKernelGGL(lk_circular_queue_kernel, dim3((unsigned)g.blocks), dim3(64), 0, stream, d_imgs, d_quads, d_pts, d_npts, cap,
                           n_frames, g.fpg, g.ppp, d_trk, d_status, prm, g.items, cur, oth);
        return;
    }
    const LkGrid g = lk_grid(n_frames, max_pts);
    hipLaunchKernelGGL(lk_circular_kernel, dim3((unsigned)g.blocks), dim3(64), 0, stream, d_imgs, d_quads, d_pts, d_npts, cap,
                       n_frames, g.fpg, g.ppp, d_trk, d_status, prm);
}

void launch_lk_hops(const PyrImage *d_imgs, const Quad *d_quads, const float2 *d_pts, const int *d_npts, int cap, int max_pts,
                    int n_frames, float2 *d_trk, uint8_t *d_status, const LkParams &prm, int hop_begin, int hop_end,
                    hipStream_t stream)
{
    if (max_pts <= 0 || n_frames <= 0 || hop_begin < 0 || hop_end > 4 || hop_begin >= hop_end)
        return;
    const LkGrid g = lk_grid(n_frames, max_pts);
    hipLaunchKernelGGL(lk_hops_kernel, dim3((unsigned)g.blocks), dim3(64), 0, stream, d_imgs, d_quads, d_pts, d_npts, cap, n_frames,
                       g.fpg, g.ppp, d_trk, d_status, prm, hop_begin, hop_end);
}

#endif // VO_HOST_EMUL

} // namespace vo

#ifdef VO_HOST_EMUL // the CPU emulator (tests/host_check) includes this file and runs the developer build's variants of it too
#include "dev/lk_dev.hip"
#endif
