// corners_response_emu.cpp -- TEST ONLY.  Executes the product's Shi-Tomasi detector with a response (visual_odom_amd/csrc/corners.hip:
// corn_map_resp_kernel<5, 0>, <3, 1>, <5, 1>, then corn_cand_kernel and corn_select_kernel; at (3, min-eigen) the two
// kernels launch_corners takes there) on the CPU through the coroutine SIMT emulator of hip_emu.h, launched block by block over the
// grids launch_corners / launch_corner_map use.  Every image AND every mask is a heap block of its own of exactly (h - 1) * stride
// + w bytes and every map and list has exactly its size, so that under AddressSanitizer a load or store outside one aborts.  Two
// forms: a shared library for tests/corners_response_cases.py, and -- with -DCORNERS_RESPONSE_EMU_MAIN -- a stand-alone program (the
// sanitizer tier: built with -fsanitize=address,undefined and run as a child, nothing instrumented is loaded into python).  Not a
// product path.
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

template <int B, int HARRIS>
void map_grid(const vo::PyrImage *tab, int first, int n, int w, float *maps, size_t map_stride, unsigned *max_key, const uint8_t *const *masks,
              int mask_pitch, double k)
{
    using namespace vo;
    constexpr int COLS = B == 5 ? CM_COLS5 : CM_COLS;
    for (int s = 0; s < n; s++)
        for (int b = 0; b < (w + COLS - 1) / COLS; b++)
            emu::run_block(CM_T, (unsigned)b, (unsigned)s, 0, [&] { corn_map_resp_kernel<B, HARRIS>(tab, first, maps, map_stride, max_key, masks, mask_pitch, k); });
}

// the map pass as launch_corners / launch_corner_map choose it
void map_pass(int block, int harris, const vo::PyrImage *tab, int first, int n, int w, float *maps, size_t map_stride, unsigned *max_key,
              const uint8_t *const *masks, int mask_pitch, double k)
{
    using namespace vo;
    if (block == 5 && !harris)
        map_grid<5, 0>(tab, first, n, w, maps, map_stride, max_key, masks, mask_pitch, k);
    else if (block == 5)
        map_grid<5, 1>(tab, first, n, w, maps, map_stride, max_key, masks, mask_pitch, k);
    else if (harris)
        map_grid<3, 1>(tab, first, n, w, maps, map_stride, max_key, masks, mask_pitch, k);
    else
        for (int s = 0; s < n; s++)
            for (int b = 0; b < (w + CM_COLS - 1) / CM_COLS; b++)
                emu::run_block(CM_T, (unsigned)b, (unsigned)s, 0, [&] {
                    if (masks)
                        corn_map_masked_kernel(tab, first, maps, map_stride, max_key, masks, mask_pitch);
                    else
                        corn_map_kernel(tab, first, maps, map_stride, max_key);
                });
}

} // namespace

extern "C" {

// the response map of one image (h rows, stride bytes apart) into out [h][w]
int cre_map(const uint8_t *img, int w, int h, int stride, int block, int harris, double k, float *out)
{
    using namespace vo;
    if (w < 1 || h < 1 || stride < w || (block != 3 && block != 5))
        return -1;
    const Planes im(img, 1, w, h, stride);
    const std::vector<PyrImage> tab = im.table(w, h, stride);
    std::unique_ptr<float[]> map(new float[(size_t)w * h]);
    map_pass(block, harris, tab.data(), 0, 1, w, map.get(), (size_t)0, nullptr, nullptr, 0, k);
    memcpy(out, map.get(), sizeof(float) * (size_t)w * h);
    return 0;
}

// The detector over images first .. first + n - 1 of a table of n_table images in one run, as launch_corners does it.  use_masks 0:
// no mask table; else image i of the table runs under masks[i] (h rows, mask_stride bytes apart) where mask_on[i] is non-zero, else
// unmasked.  lcap: the candidate-list capacity.  pts [n][cap][2], n_out [n] (-1: the list overflowed), n_cand [n], maps [n][h][w] or null.
int cre_detect(const uint8_t *imgs, const uint8_t *masks, const uint8_t *mask_on, int use_masks, int n_table, int first, int n, int w, int h, int stride,
               int mask_stride, int max_corners, double quality, double min_distance, int block, int harris, double k, int lcap, float *pts, int cap,
               int *n_out, int *n_cand, float *maps_out)
{
    using namespace vo;
    if (w < 1 || h < 1 || stride < w || n < 1 || first < 0 || first + n > n_table || lcap < 1 || !(quality > 0) || !(min_distance >= 0) ||
        (block != 3 && block != 5) || (use_masks && mask_stride < w))
        return -1;
    const Planes im(imgs, n_table, w, h, stride);
    const std::vector<PyrImage> tab = im.table(w, h, stride);
    std::unique_ptr<Planes> mk;
    std::vector<const uint8_t *> mtab;
    if (use_masks) {
        mk.reset(new Planes(masks, n_table, w, h, mask_stride));
        mtab.resize((size_t)n); // (exactly the run's slots)
        for (int s = 0; s < n; s++)
            mtab[(size_t)s] = mask_on[first + s] ? mk->blocks[(size_t)(first + s)].get() : nullptr;
    }
    const size_t S = (size_t)n;
    const int kcap = corn_pow2(lcap);
    std::vector<unsigned> max_key(S, 0u);
    std::vector<int> ncand(S, 0), nout(S, -99), status(S * lcap, 0x5a5a5a5a);
    std::vector<unsigned long long> keys(S * kcap, 0x1111111111111111ull), ckeys(S * kcap, 0x2222222222222222ull);
    std::vector<float2> out(S * lcap, make_float2(-1.f, -1.f));
    std::vector<float> maps(S * w * h, -7.f);
    CornArgs a;
    a.max_key = max_key.data();
    a.ncand = ncand.data();
    a.nout = nout.data();
    a.rounds = nullptr;
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
    a.masks = use_masks ? mtab.data() : nullptr;
    a.mask_pitch = mask_stride;
    a.block_size = block;
    a.use_harris = harris;
    a.harris_k = k;
    map_pass(block, harris, tab.data(), first, n, w, a.maps, a.map_stride, a.max_key, a.masks, a.mask_pitch, k);
    const int tiles_x = (w + CT_W - 1) / CT_W, tiles_y = (h + CT_H - 1) / CT_H;
    for (int s = 0; s < n; s++)
        for (int b = tiles_x * tiles_y - 1; b >= 0; b--) // (the append order is not part of the result: run the tiles backwards)
            emu::run_block(256, (unsigned)b, (unsigned)s, 0, [&] { corn_cand_kernel(w, h, tiles_x, a); });
    for (int s = 0; s < n; s++)
        emu::run_block(CORN_SELECT_THREADS, (unsigned)s, 0, 0, [&] { corn_select_kernel(a, w, h); });
    for (int s = 0; s < n; s++) {
        n_out[s] = nout[(size_t)s];
        n_cand[s] = ncand[(size_t)s];
        const int m = nout[(size_t)s] < cap ? nout[(size_t)s] : cap;
        if (m > 0)
            memcpy(pts + (size_t)s * cap * 2, &out[(size_t)s * lcap], sizeof(float2) * (size_t)m);
    }
    if (maps_out)
        memcpy(maps_out, maps.data(), sizeof(float) * maps.size());
    return 0;
}
}

#ifdef CORNERS_RESPONSE_EMU_MAIN
#include <stdio.h>
// in:  int32 n, w, h, stride, mask_stride, use_masks, max_corners, lcap, cap, block, harris; float64 quality, min_distance, k;
//      uint8 images [n][h][stride], masks [n][h][mask_stride], mask_on [n]
// out: float32 map of image 0 (cre_map) [h][w]; int32 n_out [n], n_cand [n]; float32 pts [n][cap][2]; float32 maps [n][h][w]
int main(int argc, char **argv)
{
    if (argc != 3)
        return 2;
    FILE *f = fopen(argv[1], "rb");
    int32_t hd[11];
    double q[3];
    if (!f || fread(hd, sizeof(hd), 1, f) != 1 || fread(q, sizeof(q), 1, f) != 1)
        return 3;
    const int n = hd[0], w = hd[1], h = hd[2], stride = hd[3], mstride = hd[4], cap = hd[8];
    std::unique_ptr<uint8_t[]> imgs(new uint8_t[(size_t)n * h * stride]), masks(new uint8_t[(size_t)n * h * mstride]), on(new uint8_t[(size_t)n]);
    if (fread(imgs.get(), 1, (size_t)n * h * stride, f) != (size_t)n * h * stride || fread(masks.get(), 1, (size_t)n * h * mstride, f) != (size_t)n * h * mstride ||
        fread(on.get(), 1, (size_t)n, f) != (size_t)n)
        return 3;
    fclose(f);
    const size_t np = (size_t)n * cap * 2, nm = (size_t)n * w * h;
    std::unique_ptr<float[]> map(new float[(size_t)w * h]), pts(new float[np > 0 ? np : 1]()), maps(new float[nm]);
    std::unique_ptr<int32_t[]> cnt(new int32_t[(size_t)2 * n]);
    if (cre_map(imgs.get(), w, h, stride, hd[9], hd[10], q[2], map.get()) != 0)
        return 4;
    if (cre_detect(imgs.get(), masks.get(), on.get(), hd[5], n, 0, n, w, h, stride, mstride, hd[6], q[0], q[1], hd[9], hd[10], q[2], hd[7], pts.get(), cap,
                   cnt.get(), cnt.get() + n, maps.get()) != 0)
        return 5;
    f = fopen(argv[2], "wb");
    if (!f || fwrite(map.get(), 4, (size_t)w * h, f) != (size_t)w * h || fwrite(cnt.get(), 4, (size_t)2 * n, f) != (size_t)2 * n ||
        fwrite(pts.get(), 4, np, f) != np || fwrite(maps.get(), 4, nm, f) != nm)
        return 6;
    fclose(f);
    return 0;
}
#endif
