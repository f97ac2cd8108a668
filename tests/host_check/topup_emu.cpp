// topup_emu.cpp -- TEST ONLY.  Executes the frame loop's detection with the top-up under a mask of the carried points
// (include/vo_topup.h) as the product launches it -- seq_prepare_kernel (seq.hip), the map pass of the frames form with a null max_key,
// corn_disc_frames_kernel, corn_max_frames_kernel, corn_cand_frames_kernel under the plane table and corn_select_frames_kernel
// (corners.hip), then bucket_kernel in its split form (fast.hip) -- on the CPU through the coroutine SIMT emulator of hip_emu.h, block by
// block over the grids launch_corners_frames_map / launch_corners_frames_masked / launch_bucket use.  Two orders:
//   inline      seq_prepare_kernel decides which frame detects again; map, discs, maximum, candidates and select run under those flags;
//   look-ahead  the map pass runs for every frame first (seq_lookahead one step early), then seq_prepare_kernel -- without counts, so
//               that it leaves n_new alone -- and the other four passes under its flags (the step).
// Every image is a heap block of its own of exactly (h - 1) * stride + w bytes, the maps are one block of exactly n w h floats (with an
// odd w h the second frame's map starts off the 16-byte grid), every plane is a block of its own of exactly w h bytes and every list
// has exactly its capacity, so that under AddressSanitizer a load or store outside one aborts.  For every frame the harness also runs
// corn_map_body with the frame's plane as its mask (the masked map kernels of the detector's own calls) into buffers of its own: the
// key corn_max_frames_kernel must reproduce.  Two forms: a shared library for tests/test_topup_emulation.py, and -- with
// -DTOPUP_EMU_MAIN -- a stand-alone program (the sanitizer tier: built with -fsanitize=address,undefined and run as a child, nothing
// instrumented is loaded into python).  Not a product path.
#include "hip_emu.h"

// (hip_emu.h has the int form only; lanes run one at a time between yields, so plain read-modify-write is atomic here)
static inline unsigned atomicMax(unsigned *p, unsigned v)
{
    const unsigned o = *p;
    *p = o > v ? o : v;
    return o;
}

#include "../../visual_odom_amd/csrc/fast.hip"
#include "../../visual_odom_amd/csrc/seq.hip"
#include "../../visual_odom_amd/csrc/corners.hip"

#include <memory>

namespace {

template <int B, int HARRIS>
void map_grid(const vo::PyrImage *tab, const vo::Quad *quads, const int *detect, int n, int w, const vo::CornArgs &a)
{
    using namespace vo;
    constexpr int COLS = B == 5 ? CM_COLS5 : CM_COLS;
    for (int s = 0; s < n; s++)
        for (int b = 0; b < (w + COLS - 1) / COLS; b++)
            emu::run_block(CM_T, (unsigned)b, (unsigned)s, 0,
                           [&] { corn_map_frames_kernel<B, HARRIS>(tab, quads, detect, a.maps, a.map_stride, nullptr, a.harris_k); });
}

// launch_corners_frames_map
void map_frames(const vo::PyrImage *tab, const vo::Quad *quads, const int *detect, int n, int w, const vo::CornArgs &a)
{
    if (a.block_size == 5 && !a.use_harris)
        map_grid<5, 0>(tab, quads, detect, n, w, a);
    else if (a.block_size == 5)
        map_grid<5, 1>(tab, quads, detect, n, w, a);
    else if (a.use_harris)
        map_grid<3, 1>(tab, quads, detect, n, w, a);
    else
        map_grid<3, 0>(tab, quads, detect, n, w, a);
}

// launch_corners_frames_masked behind its memsets and its fill
void masked_frames(const int *detect, int n, int w, int h, const vo::CornArgs &a, const vo::CornTopArgs &t)
{
    using namespace vo;
    int kept = t.max_kept < t.fcap ? t.max_kept : t.fcap;
    kept = kept > 0 ? kept : 1;
    const int disc_x = (kept + CD_WAVES - 1) / CD_WAVES;
    for (int s = 0; s < n; s++)
        for (int b = disc_x - 1; b >= 0; b--) // (every writer stores the same byte: the order is free)
            emu::run_block(CD_T, (unsigned)b, (unsigned)s, 0,
                           [&] { corn_disc_frames_kernel(t.feat, t.fcap, t.n_tracked, detect, t.radius, t.planes, w, h, disc_x); });
    const int cells = w * h;
    int wgs = (cells + CX_PER_WG - 1) / CX_PER_WG;
    wgs = wgs < 1 ? 1 : wgs > 1024 ? 1024 : wgs;
    for (int s = 0; s < n; s++)
        for (int b = wgs - 1; b >= 0; b--)
            emu::run_block(CX_T, (unsigned)b, (unsigned)s, 0, [&] { corn_max_frames_kernel(a.maps, a.map_stride, a.masks, cells, detect, a.max_key, wgs); });
    const int tiles_x = (w + CT_W - 1) / CT_W, tiles_y = (h + CT_H - 1) / CT_H;
    for (int s = 0; s < n; s++)
        for (int b = tiles_x * tiles_y - 1; b >= 0; b--)
            emu::run_block(256, (unsigned)b, (unsigned)s, 0, [&] { corn_cand_frames_kernel(w, h, tiles_x, a, detect); });
    for (int s = 0; s < n; s++)
        emu::run_block(CORN_SELECT_THREADS, (unsigned)s, 0, 0, [&] { corn_select_frames_kernel(a, w, h, detect); });
}

// corn_map_body under mask plane `mask` on table image `image`: the key of the detector's own masked calls
unsigned body_key(const vo::PyrImage *tab, int image, int w, int h, int block, int harris, double k, const uint8_t *mask)
{
    using namespace vo;
    std::unique_ptr<float[]> map(new float[(size_t)w * h]);
    unsigned key = 0;
    const uint8_t *masks[1] = {mask};
    const int cols = block == 5 ? CM_COLS5 : CM_COLS;
    for (int b = 0; b < (w + cols - 1) / cols; b++)
        emu::run_block(CM_T, (unsigned)b, 0, 0, [&] {
            if (block == 5 && !harris)
                corn_map_resp_kernel<5, 0>(tab, image, map.get(), 0, &key, masks, w, k);
            else if (block == 5)
                corn_map_resp_kernel<5, 1>(tab, image, map.get(), 0, &key, masks, w, k);
            else if (harris)
                corn_map_resp_kernel<3, 1>(tab, image, map.get(), 0, &key, masks, w, k);
            else
                corn_map_masked_kernel(tab, image, map.get(), 0, &key, masks, w);
        });
    return key;
}

} // namespace

#define TE_COUNTS 10

extern "C" {

// hd: n_table, w, h, stride, n_frames, max_corners, block, harris, lcap, bucket_size, fpb, bucket_threads, out_cap, redetect_below,
//     lookahead, radius
// q:  quality, min_distance, k
// quad_l0 [n_frames]: the table image each frame's quadruple names as its left t0 image; n_tracked [n_frames];
// carried [n_frames][lcap][2], ages [n_frames][lcap] (zero beyond the ages a frame carries); imgs [n_table][h][stride]
// counts [TE_COUNTS][n_frames]: bucketed, overflow flags, n_new, candidates, map touched, detect flag, candidate buffers touched,
//                               plane touched (a byte other than 0xFF), max_key of corn_max_frames_kernel, key of corn_map_body
// out_pts [n_frames][out_cap][2], out_ages [n_frames][out_cap], out_planes [n_frames][h][w]
int te_run(const int32_t *hd, const double *q, const int32_t *quad_l0, const int32_t *n_tracked, const float *carried, const int32_t *ages,
           const uint8_t *imgs, int32_t *counts, float *out_pts, int32_t *out_ages, uint8_t *out_planes)
{
    using namespace vo;
    const int n_table = hd[0], w = hd[1], h = hd[2], stride = hd[3], n = hd[4], lcap = hd[8], bs = hd[9], fpb = hd[10], bthreads = hd[11], out_cap = hd[12],
              redetect_below = hd[13], lookahead = hd[14], radius = hd[15];
    if (w < 1 || h < 1 || stride < w || n < 1 || n_table < 1 || lcap < 1 || out_cap < 1 || (hd[6] != 3 && hd[6] != 5) || !(q[0] > 0) || !(q[1] >= 0) ||
        (bthreads != 256 && bthreads != 1024) || !bucket_grid_ok(w, h, bs, fpb) || radius < 0 || radius > 256)
        return -1;
    std::vector<std::unique_ptr<uint8_t[]>> blocks, plane_blocks;
    std::vector<PyrImage> tab((size_t)n_table);
    const size_t bytes = (size_t)(h - 1) * stride + w, cells = (size_t)w * h;
    for (int i = 0; i < n_table; i++) {
        blocks.emplace_back(new uint8_t[bytes]);
        memcpy(blocks.back().get(), imgs + (size_t)i * h * stride, bytes);
        memset(&tab[i], 0, sizeof(PyrImage));
        tab[i].lvl[0] = blocks.back().get();
        tab[i].w[0] = w;
        tab[i].h[0] = h;
        tab[i].stride[0] = stride;
    }
    const size_t S = (size_t)n;
    std::vector<Quad> quads(S);
    std::vector<uint8_t *> planes(S);
    for (int f = 0; f < n; f++) {
        if (quad_l0[f] < 0 || quad_l0[f] >= n_table || n_tracked[f] < 0 || n_tracked[f] > lcap)
            return -1;
        quads[f] = Quad{quad_l0[f], -1, -1, -1}; // (only l0 may be read)
        plane_blocks.emplace_back(new uint8_t[cells]);
        planes[f] = plane_blocks.back().get();
        memset(planes[f], 0xFF, cells); // the fill
    }
    const int kcap = corn_pow2(lcap);
    std::vector<unsigned> max_key(S, 0u);
    std::vector<int> ncand(S, 0), n_new(S, -99), status(S * lcap, 0x5a5a5a5a), active(S, 1), detect(S, -99);
    std::vector<unsigned long long> keys(S * kcap, 0x1111111111111111ull), ckeys(S * kcap, 0x2222222222222222ull);
    std::vector<float2> corners(S * lcap, make_float2(-1.f, -1.f)), feat(S * lcap);
    std::vector<int> fages(ages, ages + S * lcap), nt(n_tracked, n_tracked + S);
    std::unique_ptr<float[]> maps(new float[S * cells]);
    for (size_t i = 0; i < S * cells; i++)
        maps[i] = -7.f;
    memcpy(feat.data(), carried, sizeof(float2) * S * lcap);
    CornArgs a;
    a.max_key = max_key.data();
    a.ncand = ncand.data();
    a.rounds = nullptr;
    a.keys = keys.data();
    a.ckeys = ckeys.data();
    a.status = status.data();
    a.pts = corners.data();
    a.nout = n_new.data();
    a.maps = maps.get();
    a.map_stride = cells;
    a.lcap = lcap;
    a.kcap = kcap;
    a.quality = q[0];
    a.max_corners = hd[5];
    a.cell = q[1] >= 1 ? (int)lrint(q[1]) : 1; // (corn_args of capi_corners.hip)
    a.lim = q[1] >= 1 ? (int)ceil(q[1] * q[1]) : 0;
    a.block_size = hd[6];
    a.use_harris = hd[7];
    a.harris_k = q[2];
    CornTopArgs t;
    t.feat = feat.data();
    t.fcap = lcap;
    t.n_tracked = nt.data();
    t.radius = radius;
    t.planes = planes.data();
    t.plane0 = nullptr; // (the fill is above)
    t.plane_stride = 0;
    t.max_kept = redetect_below - 1;
    auto prepare = [&] {
        for (int b = 0; b < (n + 63) / 64; b++)
            emu::run_block(64, (unsigned)b, 0, 0, [&] { seq_prepare_kernel(active.data(), nt.data(), redetect_below, detect.data(), nullptr, n_new.data(), n); });
    };
    if (lookahead) { // the maps one step early, for every frame
        map_frames(tab.data(), quads.data(), nullptr, n, w, a);
        prepare();
    } else {
        prepare();
        map_frames(tab.data(), quads.data(), detect.data(), n, w, a);
    }
    a.masks = planes.data();
    a.mask_pitch = w;
    masked_frames(detect.data(), n, w, h, a, t);
    std::vector<float2> bp(S * out_cap, make_float2(-2.f, -2.f));
    std::vector<int> ba(S * out_cap, -2), bn(S, -99), ovf(S, -99);
    const bool fine = (long long)(h / bs + 1) * (w / bs + 1) > BK_MAX_CELLS; // (launch_bucket's choice)
    for (int f = 0; f < n; f++)
        emu::run_block((unsigned)bthreads, (unsigned)f, 0, 0, [&] {
            if (fine)
                bucket_kernel<BK_FINE_CELLS>(feat.data(), fages.data(), nt.data(), n_new.data(), lcap, h, w, bs, fpb, bp.data(), ba.data(), bn.data(), out_cap,
                                             active.data(), ovf.data(), corners.data());
            else
                bucket_kernel<BK_MAX_CELLS>(feat.data(), fages.data(), nt.data(), n_new.data(), lcap, h, w, bs, fpb, bp.data(), ba.data(), bn.data(), out_cap,
                                            active.data(), ovf.data(), corners.data());
        });
    for (int f = 0; f < n; f++) {
        counts[0 * n + f] = bn[f];
        counts[1 * n + f] = ovf[f];
        counts[2 * n + f] = n_new[f];
        counts[3 * n + f] = ncand[f];
        bool map_touched = false, cand_touched = ncand[f] != 0 || max_key[f] != 0, plane_touched = false;
        for (size_t i = 0; i < cells && !map_touched; i++)
            map_touched = maps[(size_t)f * cells + i] != -7.f;
        for (int i = 0; i < kcap && !cand_touched; i++)
            cand_touched = keys[(size_t)f * kcap + i] != 0x1111111111111111ull || ckeys[(size_t)f * kcap + i] != 0x2222222222222222ull;
        for (size_t i = 0; i < cells && !plane_touched; i++)
            plane_touched = planes[f][i] != 0xFF;
        counts[4 * n + f] = map_touched ? 1 : 0;
        counts[5 * n + f] = detect[f];
        counts[6 * n + f] = cand_touched ? 1 : 0;
        counts[7 * n + f] = plane_touched ? 1 : 0;
        counts[8 * n + f] = (int32_t)max_key[f];
        counts[9 * n + f] = (int32_t)body_key(tab.data(), quad_l0[f], w, h, hd[6], hd[7], q[2], planes[f]);
        memcpy(out_planes + (size_t)f * cells, planes[f], cells);
    }
    memcpy(out_pts, bp.data(), sizeof(float2) * S * out_cap);
    memcpy(out_ages, ba.data(), sizeof(int) * S * out_cap);
    return 0;
}
}

#ifdef TOPUP_EMU_MAIN
#include <stdio.h>
// in:  int32 hd [16]; float64 q [3]; int32 quad_l0 [n], n_tracked [n]; float32 carried [n][lcap][2]; int32 ages [n][lcap];
//      uint8 images [n_table][h][stride]
// out: int32 counts [TE_COUNTS][n]; float32 pts [n][out_cap][2]; int32 ages [n][out_cap]; uint8 planes [n][h][w]
int main(int argc, char **argv)
{
    if (argc != 3)
        return 2;
    FILE *f = fopen(argv[1], "rb");
    int32_t hd[16];
    double q[3];
    if (!f || fread(hd, sizeof(hd), 1, f) != 1 || fread(q, sizeof(q), 1, f) != 1)
        return 3;
    const size_t n = (size_t)hd[4], lcap = (size_t)hd[8], out_cap = (size_t)hd[12], cells = (size_t)hd[1] * hd[2];
    std::vector<int32_t> quad_l0(n), nt(n), ages(n * lcap);
    std::vector<float> carried(n * lcap * 2);
    std::vector<uint8_t> imgs((size_t)hd[0] * hd[2] * hd[3]);
    if (fread(quad_l0.data(), 4, n, f) != n || fread(nt.data(), 4, n, f) != n || fread(carried.data(), 4, carried.size(), f) != carried.size() ||
        fread(ages.data(), 4, ages.size(), f) != ages.size() || fread(imgs.data(), 1, imgs.size(), f) != imgs.size())
        return 3;
    fclose(f);
    std::vector<int32_t> counts(TE_COUNTS * n), oa(n * out_cap);
    std::vector<float> op(n * out_cap * 2);
    std::vector<uint8_t> planes(n * cells);
    if (te_run(hd, q, quad_l0.data(), nt.data(), carried.data(), ages.data(), imgs.data(), counts.data(), op.data(), oa.data(), planes.data()) != 0)
        return 5;
    f = fopen(argv[2], "wb");
    if (!f || fwrite(counts.data(), 4, counts.size(), f) != counts.size() || fwrite(op.data(), 4, op.size(), f) != op.size() ||
        fwrite(oa.data(), 4, oa.size(), f) != oa.size() || fwrite(planes.data(), 1, planes.size(), f) != planes.size())
        return 6;
    fclose(f);
    return 0;
}
#endif
