// corners_emu.cpp -- TEST ONLY.  Executes the product's Shi-Tomasi detector, with and without a mask (visual_odom_amd/csrc/corners.hip:
// corn_map_kernel, corn_map_masked_kernel, corn_cand_kernel, corn_select_kernel, corn_disc_kernel) on the CPU through the coroutine
// SIMT emulator of hip_emu.h, launched block by block over the grids launch_corners / launch_corner_map / launch_corner_disc_mask
// use.  Every image AND every mask is a heap block of its own of exactly (h - 1) * stride + w bytes and every list has exactly its
// capacity, so that under AddressSanitizer a load or store outside one aborts.  Two forms: a shared library for tests/corners_emu.py
// and tests/corners_mask_cases.py, and -- with -DCORNERS_EMU_MAIN or -DCORNERS_MASK_EMU_MAIN, one main() each -- a stand-alone
// program (the sanitizer tier: built with -fsanitize=address,undefined and run as a child, nothing instrumented is loaded into
// python).  Not a product path.
#include "hip_emu.h"

// (hip_emu.h has the int form only; lanes run one at a time between yields, so plain read-modify-write is atomic here)
static inline unsigned atomicMax(unsigned *p, unsigned v)
{
    const unsigned o = *p;
    *p = o > v ? o : v;
    return o;
}

#include "../../visual_odom_amd/csrc/corners.hip"

#include <memory>

namespace {

// n planes (images or masks) of h rows, `stride` bytes apart, each copied into a block of exactly (h - 1) * stride + w bytes
struct Planes {
    std::vector<std::unique_ptr<uint8_t[]>> blocks;
    Planes(const uint8_t *src, int n, int w, int h, int stride)
    {
        const size_t bytes = (size_t)(h - 1) * stride + w;
        for (int i = 0; i < n; i++) {
            blocks.emplace_back(new uint8_t[bytes]);
            memcpy(blocks.back().get(), src + (size_t)i * h * stride, bytes);
        }
    }
    // the planes as level 0 of an image table
    std::vector<vo::PyrImage> table(int w, int h, int stride) const
    {
        std::vector<vo::PyrImage> tab(blocks.size());
        for (size_t i = 0; i < blocks.size(); i++) {
            memset(&tab[i], 0, sizeof(vo::PyrImage));
            tab[i].lvl[0] = blocks[i].get();
            tab[i].w[0] = w;
            tab[i].h[0] = h;
            tab[i].stride[0] = stride;
        }
        return tab;
    }
};

// The detector over images first .. first + n - 1 of a table of n_table images in one run, as launch_corners does it: map ->
// candidates -> select.  masks: null (corn_map_kernel), or the run's n slots (corn_map_masked_kernel; a slot's entry may be null).
// lcap: the candidate-list capacity.  pts [n][cap][2], n_out [n] (-1: the list overflowed), n_cand [n], rounds [n] or null.
int detect(const uint8_t *imgs, int n_table, int first, int n, int w, int h, int stride, const uint8_t *const *masks, int mask_stride, int max_corners,
           double quality, double min_distance, int lcap, float *pts, int cap, int *n_out, int *n_cand, int *rounds)
{
    using namespace vo;
    if (w < 1 || h < 1 || stride < w || n < 1 || first < 0 || first + n > n_table || lcap < 1 || !(quality > 0) || !(min_distance >= 0))
        return -1;
    const Planes im(imgs, n_table, w, h, stride);
    const std::vector<PyrImage> tab = im.table(w, h, stride);
    const size_t S = (size_t)n;
    const int kcap = corn_pow2(lcap);
    std::vector<unsigned> max_key(S, 0u);
    std::vector<int> ncand(S, 0), nout(S, -99), rnd(S, -99), status(S * lcap, 0x5a5a5a5a);
    std::vector<unsigned long long> keys(S * kcap, 0x1111111111111111ull), ckeys(S * kcap, 0x2222222222222222ull);
    std::vector<float2> out(S * lcap, make_float2(-1.f, -1.f));
    std::vector<float> maps(S * w * h, -7.f);
    CornArgs a;
    a.max_key = max_key.data();
    a.ncand = ncand.data();
    a.nout = nout.data();
    a.rounds = rounds ? rnd.data() : nullptr;
    a.keys = keys.data();
    a.ckeys = ckeys.data();
    a.status = status.data();
    a.pts = out.data();
    a.maps = maps.data();
    a.map_stride = (size_t)w * h;
    a.lcap = lcap;
    a.kcap = kcap;
    a.quality = quality;
    a.max_corners = max_corners;
    a.cell = min_distance >= 1 ? (int)lrint(min_distance) : 1; // (corn_args of capi_corners.hip)
    a.lim = min_distance >= 1 ? (int)ceil(min_distance * min_distance) : 0;
    a.masks = masks;
    a.mask_pitch = mask_stride;
    const int tiles_x = (w + CT_W - 1) / CT_W, tiles_y = (h + CT_H - 1) / CT_H;
    for (int s = 0; s < n; s++)
        for (int b = 0; b < (w + CM_COLS - 1) / CM_COLS; b++)
            emu::run_block(CM_T, (unsigned)b, (unsigned)s, 0, [&] {
                if (masks)
                    corn_map_masked_kernel(tab.data(), first, a.maps, a.map_stride, a.max_key, a.masks, a.mask_pitch);
                else
                    corn_map_kernel(tab.data(), first, a.maps, a.map_stride, a.max_key);
            });
    for (int s = 0; s < n; s++)
        for (int b = tiles_x * tiles_y - 1; b >= 0; b--) // (the append order is not part of the result: run the tiles backwards)
            emu::run_block(256, (unsigned)b, (unsigned)s, 0, [&] { corn_cand_kernel(w, h, tiles_x, a); });
    for (int s = 0; s < n; s++)
        emu::run_block(CORN_SELECT_THREADS, (unsigned)s, 0, 0, [&] { corn_select_kernel(a, w, h); });
    for (int s = 0; s < n; s++) {
        n_out[s] = nout[(size_t)s];
        n_cand[s] = ncand[(size_t)s];
        if (rounds)
            rounds[s] = rnd[(size_t)s];
        const int m = nout[(size_t)s] < cap ? nout[(size_t)s] : cap;
        if (m > 0)
            memcpy(pts + (size_t)s * cap * 2, &out[(size_t)s * lcap], sizeof(float2) * (size_t)m);
    }
    return 0;
}

} // namespace

extern "C" {

// cv::cornerMinEigenVal of one image (h rows, stride bytes apart) into eig [h][w]
int ce_map(const uint8_t *img, int w, int h, int stride, float *eig)
{
    using namespace vo;
    if (w < 1 || h < 1 || stride < w)
        return -1;
    const Planes im(img, 1, w, h, stride);
    const std::vector<PyrImage> tab = im.table(w, h, stride);
    std::vector<float> map((size_t)w * h, -7.f);
    for (int b = 0; b < (w + CM_COLS - 1) / CM_COLS; b++)
        emu::run_block(CM_T, (unsigned)b, 0, 0, [&] { corn_map_kernel(tab.data(), 0, map.data(), (size_t)0, nullptr); });
    memcpy(eig, map.data(), sizeof(float) * map.size());
    return 0;
}

// the detector without a mask: detect(), with the suppression rounds [n]
int ce_detect(const uint8_t *imgs, int n_table, int first, int n, int w, int h, int stride, int max_corners, double quality, double min_distance,
              int lcap, float *pts, int cap, int *n_out, int *n_cand, int *rounds)
{
    return detect(imgs, n_table, first, n, w, h, stride, nullptr, 0, max_corners, quality, min_distance, lcap, pts, cap, n_out, n_cand, rounds);
}

// the detector with a mask table: image i of the table runs under masks[i] (h rows, mask_stride bytes apart) where mask_on[i] is
// non-zero, else unmasked
int cme_detect(const uint8_t *imgs, const uint8_t *masks, const uint8_t *mask_on, int n_table, int first, int n, int w, int h, int stride,
               int mask_stride, int max_corners, double quality, double min_distance, int lcap, float *pts, int cap, int *n_out, int *n_cand)
{
    if (w < 1 || h < 1 || mask_stride < w || n < 1 || first < 0 || first + n > n_table)
        return -1;
    const Planes mk(masks, n_table, w, h, mask_stride);
    std::vector<const uint8_t *> mtab((size_t)n); // (exactly the run's slots)
    for (int s = 0; s < n; s++)
        mtab[(size_t)s] = mask_on[first + s] ? mk.blocks[(size_t)(first + s)].get() : nullptr;
    return detect(imgs, n_table, first, n, w, h, stride, mtab.data(), mask_stride, max_corners, quality, min_distance, lcap, pts, cap, n_out, n_cand,
                  nullptr);
}

// The disc mask of kept [n_kept][2] as launch_corner_disc_mask builds it: 0xFF, then the disc kernel.  mask_out: (h - 1) *
// mask_stride + w bytes (the bytes between the rows come back as the fill).
int cme_disc(const float *kept, int n_kept, int radius, int w, int h, int mask_stride, uint8_t *mask_out)
{
    using namespace vo;
    if (w < 1 || h < 1 || mask_stride < w || n_kept < 0 || radius < 0)
        return -1;
    const size_t bytes = (size_t)(h - 1) * mask_stride + w;
    std::unique_ptr<uint8_t[]> mask(new uint8_t[bytes]);
    memset(mask.get(), 0xFF, bytes);
    std::unique_ptr<float2[]> pts(new float2[(size_t)(n_kept > 0 ? n_kept : 1)]);
    for (int i = 0; i < n_kept; i++)
        pts[(size_t)i] = make_float2(kept[2 * i], kept[2 * i + 1]);
    for (int b = 0; b < (n_kept + CD_WAVES - 1) / CD_WAVES; b++)
        emu::run_block(CD_T, (unsigned)b, 0, 0, [&] { corn_disc_kernel(pts.get(), n_kept, radius, mask.get(), w, h, mask_stride); });
    memcpy(mask_out, mask.get(), bytes);
    return 0;
}
}

#ifdef CORNERS_EMU_MAIN
#include <stdio.h>
// in:  int32 n, w, h, stride, max_corners, lcap, cap; float64 quality, min_distance; uint8 images [n][h][stride]
// out: float32 map of image 0 [h][w]; int32 n_out [n], n_cand [n], rounds [n]; float32 pts [n][cap][2]
int main(int argc, char **argv)
{
    if (argc != 3)
        return 2;
    FILE *f = fopen(argv[1], "rb");
    int32_t hd[7];
    double q[2];
    if (!f || fread(hd, sizeof(hd), 1, f) != 1 || fread(q, sizeof(q), 1, f) != 1)
        return 3;
    const int n = hd[0], w = hd[1], h = hd[2], stride = hd[3], cap = hd[6];
    std::vector<uint8_t> imgs((size_t)n * h * stride);
    if (fread(imgs.data(), 1, imgs.size(), f) != imgs.size())
        return 3;
    fclose(f);
    std::vector<float> map((size_t)w * h), pts((size_t)n * cap * 2 + 1, 0.f);
    std::vector<int32_t> cnt((size_t)3 * n);
    if (ce_map(imgs.data(), w, h, stride, map.data()) != 0)
        return 4;
    if (ce_detect(imgs.data(), n, 0, n, w, h, stride, hd[4], q[0], q[1], hd[5], pts.data(), cap, cnt.data(), cnt.data() + n, cnt.data() + 2 * n) != 0)
        return 5;
    f = fopen(argv[2], "wb");
    if (!f || fwrite(map.data(), 4, map.size(), f) != map.size() || fwrite(cnt.data(), 4, cnt.size(), f) != cnt.size() ||
        fwrite(pts.data(), 4, (size_t)n * cap * 2, f) != (size_t)n * cap * 2)
        return 6;
    fclose(f);
    return 0;
}
#endif

#ifdef CORNERS_MASK_EMU_MAIN
#include <stdio.h>
// in:  int32 n, w, h, stride, mask_stride, max_corners, lcap, cap, n_kept, radius; float64 quality, min_distance;
//      uint8 images [n][h][stride], masks [n][h][mask_stride], mask_on [n]; float32 kept [n_kept][2]
// out: int32 n_out [n], n_cand [n]; float32 pts [n][cap][2]; uint8 disc mask [(h - 1) * mask_stride + w]
int main(int argc, char **argv)
{
    if (argc != 3)
        return 2;
    FILE *f = fopen(argv[1], "rb");
    int32_t hd[10];
    double q[2];
    if (!f || fread(hd, sizeof(hd), 1, f) != 1 || fread(q, sizeof(q), 1, f) != 1)
        return 3;
    const int n = hd[0], w = hd[1], h = hd[2], stride = hd[3], mstride = hd[4], cap = hd[7], n_kept = hd[8];
    std::vector<uint8_t> imgs((size_t)n * h * stride), masks((size_t)n * h * mstride), on((size_t)n);
    std::vector<float> kept((size_t)2 * n_kept + 1);
    if (fread(imgs.data(), 1, imgs.size(), f) != imgs.size() || fread(masks.data(), 1, masks.size(), f) != masks.size() ||
        fread(on.data(), 1, on.size(), f) != on.size() || fread(kept.data(), 4, (size_t)2 * n_kept, f) != (size_t)2 * n_kept)
        return 3;
    fclose(f);
    std::vector<float> pts((size_t)n * cap * 2 + 1, 0.f);
    std::vector<int32_t> cnt((size_t)2 * n);
    std::vector<uint8_t> disc((size_t)(h - 1) * mstride + w);
    if (cme_detect(imgs.data(), masks.data(), on.data(), n, 0, n, w, h, stride, mstride, hd[5], q[0], q[1], hd[6], pts.data(), cap, cnt.data(),
                   cnt.data() + n) != 0)
        return 5;
    if (cme_disc(kept.data(), n_kept, hd[9], w, h, mstride, disc.data()) != 0)
        return 5;
    f = fopen(argv[2], "wb");
    if (!f || fwrite(cnt.data(), 4, cnt.size(), f) != cnt.size() || fwrite(pts.data(), 4, (size_t)n * cap * 2, f) != (size_t)n * cap * 2 ||
        fwrite(disc.data(), 1, disc.size(), f) != disc.size())
        return 6;
    fclose(f);
    return 0;
}
#endif
