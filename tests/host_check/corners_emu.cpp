// corners_emu.cpp -- TEST ONLY.  Executes the product's Shi-Tomasi detector (visual_odom_amd/csrc/corners.hip: corn_map_kernel,
// corn_cand_kernel, corn_select_kernel) on the CPU through the coroutine SIMT emulator of hip_emu.h, launched block by block over the
// grids launch_corners / launch_corner_map use.  Every image is a heap block of its own of exactly (h - 1) * stride + w bytes and
// every list has exactly its capacity, so that under AddressSanitizer a load or store outside one aborts.  Two forms: a shared
// library for tests/corners_emu.py, and -- with -DCORNERS_EMU_MAIN -- a stand-alone program (the sanitizer tier: built with
// -fsanitize=address,undefined and run as a child, nothing instrumented is loaded into python).  Not a product path.
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

struct Images {
    std::vector<std::unique_ptr<uint8_t[]>> blocks;
    std::vector<vo::PyrImage> tab;
    // imgs: n images of h rows, `stride` bytes apart (the last row holds w bytes)
    Images(const uint8_t *imgs, int n, int w, int h, int stride)
    {
        const size_t bytes = (size_t)(h - 1) * stride + w;
        tab.resize((size_t)n);
        for (int i = 0; i < n; i++) {
            blocks.emplace_back(new uint8_t[bytes]);
            memcpy(blocks.back().get(), imgs + (size_t)i * h * stride, bytes);
            memset(&tab[(size_t)i], 0, sizeof(vo::PyrImage));
            tab[(size_t)i].lvl[0] = blocks.back().get();
            tab[(size_t)i].w[0] = w;
            tab[(size_t)i].h[0] = h;
            tab[(size_t)i].stride[0] = stride;
        }
    }
};

} // namespace

extern "C" {

// cv::cornerMinEigenVal of one image (h rows, stride bytes apart) into eig [h][w]
int ce_map(const uint8_t *img, int w, int h, int stride, float *eig)
{
    using namespace vo;
    if (w < 1 || h < 1 || stride < w)
        return -1;
    Images im(img, 1, w, h, stride);
    std::vector<float> map((size_t)w * h, -7.f);
    for (int b = 0; b < (w + CM_COLS - 1) / CM_COLS; b++)
        emu::run_block(CM_T, (unsigned)b, 0, 0, [&] { corn_map_kernel(im.tab.data(), 0, map.data(), (size_t)0, nullptr); });
    memcpy(eig, map.data(), sizeof(float) * map.size());
    return 0;
}

// The detector over images first .. first + n - 1 of a table of n_table images in one run, as launch_corners does it.  lcap: the
// candidate-list capacity.  pts [n][cap][2], n_out [n] (-1: the list overflowed), n_cand [n], rounds [n].
int ce_detect(const uint8_t *imgs, int n_table, int first, int n, int w, int h, int stride, int max_corners, double quality, double min_distance,
              int lcap, float *pts, int cap, int *n_out, int *n_cand, int *rounds)
{
    using namespace vo;
    if (w < 1 || h < 1 || stride < w || n < 1 || first < 0 || first + n > n_table || lcap < 1 || !(quality > 0) || !(min_distance >= 0))
        return -1;
    Images im(imgs, n_table, w, h, stride);
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
    a.rounds = rnd.data();
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
    const int tiles_x = (w + CT_W - 1) / CT_W, tiles_y = (h + CT_H - 1) / CT_H;
    for (int s = 0; s < n; s++)
        for (int b = 0; b < (w + CM_COLS - 1) / CM_COLS; b++)
            emu::run_block(CM_T, (unsigned)b, (unsigned)s, 0, [&] { corn_map_kernel(im.tab.data(), first, a.maps, a.map_stride, a.max_key); });
    for (int s = 0; s < n; s++)
        for (int b = tiles_x * tiles_y - 1; b >= 0; b--) // (the append order is not part of the result: run the tiles backwards)
            emu::run_block(256, (unsigned)b, (unsigned)s, 0, [&] { corn_cand_kernel(w, h, tiles_x, a); });
    for (int s = 0; s < n; s++)
        emu::run_block(CORN_SELECT_THREADS, (unsigned)s, 0, 0, [&] { corn_select_kernel(a, w, h); });
    for (int s = 0; s < n; s++) {
        n_out[s] = nout[(size_t)s];
        n_cand[s] = ncand[(size_t)s];
        rounds[s] = rnd[(size_t)s];
        const int m = nout[(size_t)s] < cap ? nout[(size_t)s] : cap;
        if (m > 0)
            memcpy(pts + (size_t)s * cap * 2, &out[(size_t)s * lcap], sizeof(float2) * (size_t)m);
    }
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
