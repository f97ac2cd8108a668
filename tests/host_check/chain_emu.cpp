// chain_emu.cpp -- TEST ONLY.  The 4-hop chain kernels of lk.hip (lk_circular_kernel, lk_hops_kernel) over a BATCH of frames on the
// CPU, through the coroutine SIMT emulator of hip_emu.h: pyr_pass_kernel (pyramid.hip) over an image table, then the chain over
// the product's lk_grid -- the frame -> XCD numbering with parts of a frame's list (fewer than 8 frames) and a partial last group
// included, which kernel_emu.cpp's one-frame launch does not reach.  Every level of every pyramid is a heap block of its own of
// exactly stride x (h + 2 VO_BY) bytes / dwords (emu_pyramid.h): under AddressSanitizer a tile fill or a template read outside a
// level aborts.  Two forms: a shared library for tests/lk_chain_cases.py and -- with -DCHAIN_EMU_MAIN -- a stand-alone program
// (built with -fsanitize=address,undefined and run as a child; nothing instrumented is loaded into python).  Not a product path.
#include "hip_emu.h"

#include "../../visual_odom_amd/csrc/lk.hip"
#include "../../visual_odom_amd/csrc/pyramid.hip"

#include "emu_pyramid.h"

extern "C" {

// imgs: n_img tight w x h gray images; quads [n_frames][4]: indices (l0, r0, l1, r1) into them; pts [n_frames][n][2], frame f
// tracks its first counts[f]; split: 0 = one launch of lk_circular_kernel, 1 = lk_hops_kernel [0, 1) + [1, 4) over outputs that
// start as garbage.  trk [n_frames][4][n][2], status [n_frames][4][n]; rows from counts[f] on come back untouched (123456, -7 /
// 0xA5).  Returns the number of pyramid levels built.
int ce_chain(const uint8_t *imgs, int n_img, int w, int h, int max_level, const int *quads, int n_frames, const float *pts, const int *counts,
             int n, int full_chain, int split, float *trk, uint8_t *status)
{
    using namespace vo;
    const Plan p = plan(w, h, max_level);
    std::vector<const uint8_t *> img_ptr;
    for (int i = 0; i < n_img; i++)
        img_ptr.push_back(imgs + (size_t)i * w * h);
    Heap heap(p, img_ptr.data(), n_img, w, h);
    const PyrImage *d_imgs = heap.tab.data();
    const PassPlan pp = pass_plan(p.levels, p.lw, p.lh, p.ls, /*wide border items*/ false);
    for (int l = 0; l < p.levels; l++) {
        const uint32_t nwg = pass_grid(pp, l, (uint32_t)n_img, 0);
        for (uint32_t b = 0; b < nwg; b++)
            emu::run_block(64, b, 0, 0, [&] { pyr_pass_kernel(d_imgs, l, p.levels, pp, (uint32_t)n_img, 0); });
    }
    LkParams prm;
    prm.max_level = p.levels - 1;
    prm.max_count = 30;
    prm.epsilon = 0.01 * 0.01;
    prm.min_eig = 1e-3f;
    prm.full_chain = full_chain;
    const int cap = n + 3; // (cap != n: the frame stride of the outputs is the capacity)
    std::vector<Quad> q((size_t)n_frames);
    std::vector<int> npts((size_t)n_frames);
    int most = 0;
    for (int f = 0; f < n_frames; f++) {
        q[(size_t)f] = Quad{quads[4 * f], quads[4 * f + 1], quads[4 * f + 2], quads[4 * f + 3]};
        npts[(size_t)f] = counts[f] < 0 ? 0 : counts[f] > n ? n : counts[f];
        most = npts[(size_t)f] > most ? npts[(size_t)f] : most;
    }
    std::vector<float2> in((size_t)n_frames * cap), out((size_t)n_frames * 4 * cap, make_float2(123456.f, -7.f));
    std::vector<uint8_t> st((size_t)n_frames * 4 * cap, (uint8_t)0xA5);
    for (int f = 0; f < n_frames; f++)
        memcpy(&in[(size_t)f * cap], pts + (size_t)f * 2 * n, sizeof(float2) * (size_t)n);
    if (most > 0) {
        const LkGrid g = lk_grid(n_frames, most);
        const int cut[3] = {0, split ? 1 : 4, 4};
        for (int k = 0; k < (split ? 2 : 1); k++)
            for (int b = 0; b < g.blocks; b++)
                emu::run_block(64, (unsigned)b, 0, 0, [&] {
                    if (split)
                        lk_hops_kernel(d_imgs, q.data(), in.data(), npts.data(), cap, n_frames, g.fpg, g.ppp, out.data(), st.data(), prm, cut[k],
                                       cut[k + 1]);
                    else
                        lk_circular_kernel(d_imgs, q.data(), in.data(), npts.data(), cap, n_frames, g.fpg, g.ppp, out.data(), st.data(), prm);
                });
    }
    for (int f = 0; f < n_frames; f++)
        for (int hop = 0; hop < 4; hop++) {
            memcpy(trk + ((size_t)f * 4 + hop) * 2 * n, &out[((size_t)f * 4 + hop) * cap], sizeof(float2) * (size_t)n);
            memcpy(status + ((size_t)f * 4 + hop) * n, &st[((size_t)f * 4 + hop) * cap], (size_t)n);
        }
    return p.levels;
}
}

#ifdef CHAIN_EMU_MAIN
#include <stdio.h>
// in:  int32 w, h, max_level, n_img, n_frames, n, full_chain, split; uint8 imgs [n_img][h][w]; int32 quads [n_frames][4];
//      int32 counts [n_frames]; float32 pts [n_frames][n][2]
// out: float32 trk [n_frames][4][n][2]; uint8 status [n_frames][4][n]
int main(int argc, char **argv)
{
    if (argc != 3)
        return 2;
    FILE *f = fopen(argv[1], "rb");
    int32_t hd[8];
    if (!f || fread(hd, sizeof(hd), 1, f) != 1)
        return 3;
    const int w = hd[0], h = hd[1], n_img = hd[3], F = hd[4], n = hd[5];
    std::vector<uint8_t> imgs((size_t)n_img * w * h), st((size_t)F * 4 * n + 1);
    std::vector<int32_t> quads((size_t)F * 4), counts((size_t)F);
    std::vector<float> pts((size_t)F * 2 * n + 2), trk((size_t)F * 8 * n + 2);
    if (fread(imgs.data(), 1, imgs.size(), f) != imgs.size() || fread(quads.data(), 4, quads.size(), f) != quads.size() ||
        fread(counts.data(), 4, counts.size(), f) != counts.size() || fread(pts.data(), 8, (size_t)F * n, f) != (size_t)F * n)
        return 3;
    fclose(f);
    if (ce_chain(imgs.data(), n_img, w, h, hd[2], quads.data(), F, pts.data(), counts.data(), n, hd[6], hd[7], trk.data(), st.data()) < 1)
        return 4;
    f = fopen(argv[2], "wb");
    if (!f || fwrite(trk.data(), 8, (size_t)F * 4 * n, f) != (size_t)F * 4 * n || fwrite(st.data(), 1, (size_t)F * 4 * n, f) != (size_t)F * 4 * n)
        return 6;
    fclose(f);
    return 0;
}
#endif
