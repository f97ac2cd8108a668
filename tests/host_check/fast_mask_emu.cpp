// fast_mask_emu.cpp -- TEST ONLY.  Executes cv::FAST under a mask (include/vo_fast_mask.h) as the product launches it, on the CPU
// through the coroutine SIMT emulator of hip_emu.h.  Two entry points:
//   fme_filter  fast_mask_filter_kernel (fast.hip) alone over caller-made corner lists and planes, at 256 or 1024 threads;
//   fme_route   the frame loop's detection with the record on: seq_prepare_kernel (seq.hip), fast_tile_kernel / fast_rowscan_kernel /
//               fast_nms_write_kernel into a list of its own (launch_fast_corners with a null n_tracked), corn_disc_frames_kernel
//               (corners.hip) over planes that hold 0xFF, fast_mask_filter_kernel, bucket_kernel in its split form -- block by block
//               over the grids launch_fast_corners / launch_corner_disc_frames / launch_fast_mask_filter / launch_bucket use.  Two
//               orders: inline (the flags first, FAST under them) and look-ahead (FAST of every frame first, as seq_lookahead makes
//               the list one step early; the flags, the discs and the filter once the carried sets are known).
// Every image level is a heap block of its own (emu_pyramid.h), every plane a block of exactly (h - 1) * pitch + w bytes and every
// list has exactly its capacity, so that under AddressSanitizer a load or store outside one aborts.  Two forms: a shared library for
// tests/test_fast_mask_emulation.py, and -- with -DFAST_MASK_EMU_MAIN -- a stand-alone program (the sanitizer tier: built with
// -fsanitize=address,undefined and run as a child, nothing instrumented is loaded into python).  Not a product path.
#include "hip_emu.h"

// (hip_emu.h has the int form only; lanes run one at a time between yields, so plain read-modify-write is atomic here)
static inline unsigned atomicMax(unsigned *p, unsigned v)
{
    const unsigned o = *p;
    *p = o > v ? o : v;
    return o;
}

#include "../../visual_odom_amd/csrc/fast.hip"
#include "../../visual_odom_amd/csrc/lk.hip"
#include "../../visual_odom_amd/csrc/pyramid.hip"
#include "../../visual_odom_amd/csrc/seq.hip"
#include "../../visual_odom_amd/csrc/corners.hip"

#include "emu_pyramid.h"

namespace {

template <typename F>
void launch(unsigned gx, unsigned gy, unsigned gz, int threads, F body)
{
    for (unsigned z = 0; z < gz; z++)
        for (unsigned y = 0; y < gy; y++)
            for (unsigned x = 0; x < gx; x++)
                emu::run_block(threads, x, y, z, body);
}

// planes [n][h][pitch] into exact blocks
struct Planes {
    std::vector<std::unique_ptr<uint8_t[]>> blocks;
    std::vector<uint8_t *> tab;
    size_t bytes;
    Planes(int n, int w, int h, int pitch, const uint8_t *src) : bytes((size_t)(h - 1) * pitch + w)
    {
        for (int f = 0; f < n; f++) {
            blocks.emplace_back(new uint8_t[bytes]);
            if (src)
                memcpy(blocks.back().get(), src + (size_t)f * h * pitch, bytes);
            else
                memset(blocks.back().get(), 0xFF, bytes); // the fill
            tab.push_back(blocks.back().get());
        }
    }
};

} // namespace

#define FME_COUNTS 6

extern "C" {

// hd: n_frames, cap, w, h, pitch, threads
// in_pts [n][cap][2], n_in [n] (may exceed cap), planes [n][h][pitch], detect [n]; out_pts [n][cap][2] in / out (what the kernel leaves
// alone comes back as it went in), n_out [n] in / out
int fme_filter(const int32_t *hd, const float *in_pts, const int32_t *n_in, const uint8_t *planes, const int32_t *detect, float *out_pts, int32_t *n_out)
{
    using namespace vo;
    const int n = hd[0], cap = hd[1], w = hd[2], h = hd[3], pitch = hd[4], threads = hd[5];
    if (n < 1 || cap < 1 || w < 1 || h < 1 || pitch < w || (threads != 256 && threads != 1024))
        return -1;
    Planes P(n, w, h, pitch, planes);
    const size_t S = (size_t)n;
    std::unique_ptr<float2[]> in(new float2[S * cap]), out(new float2[S * cap]);
    std::unique_ptr<int[]> nin(new int[S]), nout(new int[S]), det(new int[S]);
    memcpy(in.get(), in_pts, sizeof(float2) * S * cap);
    memcpy(out.get(), out_pts, sizeof(float2) * S * cap);
    for (int f = 0; f < n; f++) {
        nin[f] = n_in[f];
        nout[f] = n_out[f];
        det[f] = detect[f];
    }
    launch((unsigned)n, 1, 1, threads, [&] { fast_mask_filter_kernel(in.get(), nin.get(), cap, P.tab.data(), pitch, det.get(), out.get(), nout.get()); });
    memcpy(out_pts, out.get(), sizeof(float2) * S * cap);
    for (int f = 0; f < n; f++)
        n_out[f] = nout[f];
    return 0;
}

// hd: n_table, w, h, n_frames, threshold, nonmax, lcap, bucket_size, fpb, bucket_threads, out_cap, redetect_below, lookahead, radius,
//     filter_threads, 0
// quad_l0 [n_frames]: the table image each frame's quadruple names as its left t0 image; n_tracked [n_frames];
// carried [n_frames][lcap][2], ages [n_frames][lcap] (zero beyond the ages a frame carries); imgs [n_table][h][w]
// counts [FME_COUNTS][n_frames]: bucketed, overflow flags, n_new (the masked list), n_raw (the unmasked list), detect flag, plane touched
// out_pts [n_frames][out_cap][2], out_ages [n_frames][out_cap], out_planes [n_frames][h][w], out_new [n_frames][lcap][2] the masked lists
int fme_route(const int32_t *hd, const int32_t *quad_l0, const int32_t *n_tracked, const float *carried, const int32_t *ages, const uint8_t *imgs,
              int32_t *counts, float *out_pts, int32_t *out_ages, uint8_t *out_planes, float *out_new)
{
    using namespace vo;
    const int n_table = hd[0], w = hd[1], h = hd[2], n = hd[3], threshold = hd[4], nonmax = hd[5], lcap = hd[6], bs = hd[7], fpb = hd[8], bthreads = hd[9],
              out_cap = hd[10], redetect_below = hd[11], lookahead = hd[12], radius = hd[13], fthreads = hd[14];
    if (w < 7 || h < 7 || n < 1 || n_table < 1 || lcap < 1 || out_cap < 1 || (bthreads != 256 && bthreads != 1024) || (fthreads != 256 && fthreads != 1024) ||
        !bucket_grid_ok(w, h, bs, fpb) || radius < 0 || radius > 256)
        return -1;
    std::vector<const uint8_t *> src((size_t)n_table);
    for (int i = 0; i < n_table; i++)
        src[i] = imgs + (size_t)i * w * h;
    Heap heap(plan(w, h, 0), src.data(), n_table, w, h); // (one-level pyramids: FAST reads level 0 only)
    const size_t S = (size_t)n, cells = (size_t)w * h;
    std::vector<Quad> quads(S);
    for (int f = 0; f < n; f++) {
        if (quad_l0[f] < 0 || quad_l0[f] >= n_table || n_tracked[f] < 0 || n_tracked[f] > lcap)
            return -1;
        quads[f] = Quad{quad_l0[f], -1, -1, -1}; // (only l0 may be read)
    }
    Planes P(n, w, h, w, nullptr);
    const int segs = (w + 63) / 64;
    std::vector<int> rowcnt(S * h, 0), rowoff(S * h, -1), n_raw(S, -99), n_new(S, -99), active(S, 1), detect(S, -99);
    std::vector<unsigned long long> nmsmask(S * h * segs, 0xDEADBEEFDEADBEEFull);
    std::unique_ptr<float2[]> raw(new float2[S * lcap]), filt(new float2[S * lcap]), feat(new float2[S * lcap]);
    for (size_t i = 0; i < S * lcap; i++)
        raw[i] = filt[i] = make_float2(-1.f, -1.f);
    memcpy(feat.get(), carried, sizeof(float2) * S * lcap);
    std::vector<int> fages(ages, ages + S * lcap), nt(n_tracked, n_tracked + S);
    auto prepare = [&] {
        launch((unsigned)(n + 63) / 64, 1, 1, 64, [&] { seq_prepare_kernel(active.data(), nt.data(), redetect_below, detect.data(), nullptr, n_new.data(), n); });
    };
    auto fast = [&](const int *flags) { // launch_fast_corners with a null n_tracked
        if (n >= 8)
            launch((unsigned)segs, (unsigned)(h + 31) / 32, (unsigned)n, 256,
                   [&] { fast_tile_tall_kernel(heap.tab.data(), quads.data(), flags, threshold, nonmax, nmsmask.data(), segs, rowcnt.data()); });
        else
            launch((unsigned)segs, (unsigned)(h + 15) / 16, (unsigned)n, 256,
                   [&] { fast_tile_kernel(heap.tab.data(), quads.data(), flags, threshold, nonmax, nmsmask.data(), segs, rowcnt.data()); });
        launch((unsigned)n, 1, 1, 256, [&] { fast_rowscan_kernel(rowcnt.data(), rowoff.data(), h, flags, n_raw.data()); });
        const int rows_per_wg = 4 * fast_nms_rows_per_wave(segs);
        launch((unsigned)(h + rows_per_wg - 1) / rows_per_wg, (unsigned)n, 1, 256,
               [&] { fast_nms_write_kernel(nmsmask.data(), segs, h, flags, rowoff.data(), nullptr, lcap, raw.get()); });
    };
    if (lookahead) { // the list one step early, for every frame
        fast(nullptr);
        prepare();
    } else {
        prepare();
        fast(detect.data());
    }
    // launch_corner_disc_frames behind its fill
    int kept = redetect_below - 1 < lcap ? redetect_below - 1 : lcap;
    kept = kept > 0 ? kept : 1;
    const int disc_x = (kept + CD_WAVES - 1) / CD_WAVES;
    for (int s = 0; s < n; s++)
        for (int b = disc_x - 1; b >= 0; b--) // (every writer stores the same byte: the order is free)
            emu::run_block(CD_T, (unsigned)b, (unsigned)s, 0,
                           [&] { corn_disc_frames_kernel(feat.get(), lcap, nt.data(), detect.data(), radius, P.tab.data(), w, h, disc_x); });
    launch((unsigned)n, 1, 1, fthreads, [&] { fast_mask_filter_kernel(raw.get(), n_raw.data(), lcap, P.tab.data(), w, detect.data(), filt.get(), n_new.data()); });
    std::vector<float2> bp(S * out_cap, make_float2(-2.f, -2.f));
    std::vector<int> ba(S * out_cap, -2), bn(S, -99), ovf(S, -99);
    const bool fine = (long long)(h / bs + 1) * (w / bs + 1) > BK_MAX_CELLS; // (launch_bucket's choice)
    launch((unsigned)n, 1, 1, bthreads, [&] {
        if (fine)
            bucket_kernel<BK_FINE_CELLS>(feat.get(), fages.data(), nt.data(), n_new.data(), lcap, h, w, bs, fpb, bp.data(), ba.data(), bn.data(), out_cap,
                                         active.data(), ovf.data(), filt.get());
        else
            bucket_kernel<BK_MAX_CELLS>(feat.get(), fages.data(), nt.data(), n_new.data(), lcap, h, w, bs, fpb, bp.data(), ba.data(), bn.data(), out_cap,
                                        active.data(), ovf.data(), filt.get());
    });
    for (int f = 0; f < n; f++) {
        counts[0 * n + f] = bn[f];
        counts[1 * n + f] = ovf[f];
        counts[2 * n + f] = n_new[f];
        counts[3 * n + f] = n_raw[f];
        counts[4 * n + f] = detect[f];
        bool touched = false;
        for (size_t i = 0; i < cells && !touched; i++)
            touched = P.tab[f][i] != 0xFF;
        counts[5 * n + f] = touched ? 1 : 0;
        memcpy(out_planes + (size_t)f * cells, P.tab[f], cells);
    }
    memcpy(out_pts, bp.data(), sizeof(float2) * S * out_cap);
    memcpy(out_ages, ba.data(), sizeof(int) * S * out_cap);
    memcpy(out_new, filt.get(), sizeof(float2) * S * lcap);
    return 0;
}
}

#ifdef FAST_MASK_EMU_MAIN
#include <stdio.h>
// argv: mode ("filter" | "route"), input file, output file
// filter in:  int32 hd [6]; float32 in_pts [n][cap][2]; int32 n_in [n]; uint8 planes [n][h][pitch]; int32 detect [n];
//             float32 out_pts [n][cap][2]; int32 n_out [n]
//        out: float32 out_pts [n][cap][2]; int32 n_out [n]
// route  in:  int32 hd [16]; int32 quad_l0 [n], n_tracked [n]; float32 carried [n][lcap][2]; int32 ages [n][lcap]; uint8 images [n_table][h][w]
//        out: int32 counts [FME_COUNTS][n]; float32 pts [n][out_cap][2]; int32 ages [n][out_cap]; uint8 planes [n][h][w]; float32 new [n][lcap][2]
template <typename T>
static bool rd(FILE *f, std::vector<T> &v)
{
    return v.empty() || fread(v.data(), sizeof(T), v.size(), f) == v.size();
}
template <typename T>
static bool wr(FILE *f, const std::vector<T> &v)
{
    return v.empty() || fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
}
int main(int argc, char **argv)
{
    if (argc != 4)
        return 2;
    FILE *f = fopen(argv[2], "rb");
    if (!f)
        return 3;
    if (!strcmp(argv[1], "filter")) {
        std::vector<int32_t> hd(6);
        if (!rd(f, hd))
            return 3;
        const size_t n = (size_t)hd[0], cap = (size_t)hd[1], h = (size_t)hd[3], pitch = (size_t)hd[4];
        std::vector<float> in(n * cap * 2), out(n * cap * 2);
        std::vector<int32_t> nin(n), det(n), nout(n);
        std::vector<uint8_t> planes(n * h * pitch);
        if (!rd(f, in) || !rd(f, nin) || !rd(f, planes) || !rd(f, det) || !rd(f, out) || !rd(f, nout))
            return 3;
        fclose(f);
        if (fme_filter(hd.data(), in.data(), nin.data(), planes.data(), det.data(), out.data(), nout.data()) != 0)
            return 5;
        f = fopen(argv[3], "wb");
        if (!f || !wr(f, out) || !wr(f, nout))
            return 6;
        fclose(f);
        return 0;
    }
    std::vector<int32_t> hd(16);
    if (!rd(f, hd))
        return 3;
    const size_t n = (size_t)hd[3], lcap = (size_t)hd[6], out_cap = (size_t)hd[10], cells = (size_t)hd[1] * hd[2];
    std::vector<int32_t> quad_l0(n), nt(n), ages(n * lcap);
    std::vector<float> carried(n * lcap * 2);
    std::vector<uint8_t> imgs((size_t)hd[0] * cells);
    if (!rd(f, quad_l0) || !rd(f, nt) || !rd(f, carried) || !rd(f, ages) || !rd(f, imgs))
        return 3;
    fclose(f);
    std::vector<int32_t> counts(FME_COUNTS * n), oa(n * out_cap);
    std::vector<float> op(n * out_cap * 2), on(n * lcap * 2);
    std::vector<uint8_t> planes(n * cells);
    if (fme_route(hd.data(), quad_l0.data(), nt.data(), carried.data(), ages.data(), imgs.data(), counts.data(), op.data(), oa.data(), planes.data(), on.data()) != 0)
        return 5;
    f = fopen(argv[3], "wb");
    if (!f || !wr(f, counts) || !wr(f, op) || !wr(f, oa) || !wr(f, planes) || !wr(f, on))
        return 6;
    fclose(f);
    return 0;
}
#endif
