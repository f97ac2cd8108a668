// flow_emu.cpp -- TEST ONLY.  Executes the product's two-image tracker on the CPU through the coroutine SIMT emulator of hip_emu.h:
// pyr_pass_kernel (pyramid.hip) over the two images, lk_flow_kernel (lk.hip) over the points, flow_compact_kernel (post.hip) over
// the result.  Every level of both pyramids is a heap block of its own of exactly stride x (h + 2 VO_BY) bytes / dwords, so that
// under AddressSanitizer a load outside a level aborts (the err epilogue's tile refill included).  Two forms: a shared library
// for tests/test_flow_emulation.py, and -- with -DFLOW_EMU_MAIN -- a stand-alone program (the sanitizer tier: built with
// -fsanitize=address,undefined and run as a child, nothing instrumented is loaded into python) that reads one case from a file
// and writes the results to another.  Not a product path.
#include "hip_emu.h"

#include "../../visual_odom_amd/csrc/lk.hip"
#include "../../visual_odom_amd/csrc/pyramid.hip"
#include "../../visual_odom_amd/csrc/post.hip"

#include <memory>
#include <vector>

namespace {

// the geometry libvo_hip plans (capi.hip: plan_levels / level_stride)
struct Plan {
    int levels = 0;
    int lw[VO_MAX_LEVELS], lh[VO_MAX_LEVELS], ls[VO_MAX_LEVELS];
};

Plan plan(int w, int h, int max_level)
{
    Plan p;
    int cw = w, ch = h, l = 0;
    for (;; l++) {
        p.lw[l] = cw;
        p.lh[l] = ch;
        p.ls[l] = (VO_BX + cw + VO_BY + 15) / 16 * 16;
        const int nw = (cw + 1) / 2, nh = (ch + 1) / 2;
        if (l == max_level || l + 1 >= VO_MAX_LEVELS || nw <= 21 || nh <= 21)
            break;
        cw = nw;
        ch = nh;
    }
    p.levels = l + 1;
    return p;
}

struct Heap {
    std::vector<std::unique_ptr<uint8_t[]>> pix;
    std::vector<std::unique_ptr<uint32_t[]>> der;
    std::vector<vo::PyrImage> tab;
    Heap(const Plan &p, const uint8_t *const *imgs, int n_img, int w, int h) : tab((size_t)n_img)
    {
        for (int i = 0; i < n_img; i++) {
            memset(&tab[i], 0, sizeof(vo::PyrImage));
            for (int l = 0; l < p.levels; l++) {
                const size_t n = (size_t)p.ls[l] * (p.lh[l] + 2 * VO_BY), org = (size_t)VO_BY * p.ls[l] + VO_BX;
                pix.emplace_back(new uint8_t[n]);
                der.emplace_back(new uint32_t[n]);
                memset(pix.back().get(), 0xA5, n); // (a read of border the build did not write shows up)
                memset(der.back().get(), 0, 4 * n);
                tab[i].lvl[l] = pix.back().get() + org;
                tab[i].der[l] = der.back().get() + org;
                tab[i].w[l] = p.lw[l];
                tab[i].h[l] = p.lh[l];
                tab[i].stride[l] = p.ls[l];
            }
            for (int y = 0; y < h; y++)
                memcpy(tab[i].lvl[0] + (ptrdiff_t)y * p.ls[0], imgs[i] + (size_t)y * w, (size_t)w);
        }
    }
};

} // namespace

extern "C" {

// prev, next: tight w x h gray images; pts [n][2].  next_out [n][2], status [n], err [n] or null (the kernel's "not requested").
// n_frames copies of the pair are tracked as frames of one launch (every frame must give the same bits: frame -> XCD numbering);
// the outputs are those of frame `frame`.  Returns the number of pyramid levels built.
int fe_track(const uint8_t *prev, const uint8_t *next, int w, int h, int max_level, const float *pts, int n, int max_count, double eps,
             float min_eig, float *next_out, uint8_t *status, float *err, int n_frames, int frame)
{
    using namespace vo;
    const Plan p = plan(w, h, max_level);
    const uint8_t *imgs[2] = {prev, next};
    Heap heap(p, imgs, 2, w, h);
    const PyrImage *d_imgs = heap.tab.data();
    const PassPlan pp = pass_plan(p.levels, p.lw, p.lh, p.ls, /*wide border items*/ false);
    for (int l = 0; l < p.levels; l++) {
        const uint32_t nwg = pass_grid(pp, l, 2, 0);
        for (uint32_t b = 0; b < nwg; b++)
            emu::run_block(64, b, 0, 0, [&] { pyr_pass_kernel(d_imgs, l, p.levels, pp, 2u, 0); });
    }
    if (n <= 0)
        return p.levels;
    LkParams prm;
    prm.max_level = p.levels - 1;
    prm.max_count = max_count;
    prm.epsilon = eps * eps;
    prm.min_eig = min_eig;
    prm.full_chain = 0;
    const int cap = n + 3; // (cap != n: the frame stride of the outputs is the capacity)
    std::vector<Quad> pairs((size_t)n_frames, Quad{0, 1, 1, 0});
    std::vector<int> npts((size_t)n_frames, n);
    std::vector<float2> in((size_t)n_frames * cap), out((size_t)n_frames * cap, make_float2(123456.f, -7.f));
    std::vector<uint8_t> st((size_t)n_frames * cap, (uint8_t)0xA5);
    std::vector<float> er((size_t)n_frames * cap, -1.f);
    for (int f = 0; f < n_frames; f++)
        memcpy(&in[(size_t)f * cap], pts, sizeof(float2) * (size_t)n);
    // launch_lk_flow's grid
    const int fpg = n_frames >= 8 ? 8 : n_frames >= 4 ? 4 : n_frames >= 2 ? 2 : 1;
    const int parts = 8 / fpg, ppp = (n + parts - 1) / parts, groups = (n_frames + fpg - 1) / fpg;
    for (unsigned b = 0; b < (unsigned)(8 * groups * ppp); b++)
        emu::run_block(64, b, 0, 0, [&] {
            lk_flow_kernel(d_imgs, pairs.data(), in.data(), npts.data(), cap, n_frames, fpg, ppp, out.data(), st.data(),
                           err ? er.data() : nullptr, prm);
        });
    memcpy(next_out, &out[(size_t)frame * cap], sizeof(float2) * (size_t)n);
    memcpy(status, &st[(size_t)frame * cap], (size_t)n);
    if (err)
        memcpy(err, &er[(size_t)frame * cap], sizeof(float) * (size_t)n);
    return p.levels;
}

// flow_compact_kernel over one frame by a workgroup of `threads` threads.  status [n] is rewritten; out0 / out1 [n][2], idx [n]
int fe_compact(const float *pts0, const float *next, uint8_t *status, int n, float *out0, float *out1, int32_t *idx, int threads)
{
    const int cap = n > 1 ? n : 1;
    int n_pts = n, n_out = -1;
    emu::run_block(threads, 0, 0, 0, [&] {
        vo::flow_compact_kernel((const float2 *)pts0, (const float2 *)next, status, &n_pts, cap, (float2 *)out0, (float2 *)out1, idx, &n_out);
    });
    return n_out;
}
}

#ifdef FLOW_EMU_MAIN
#include <stdio.h>
// in:  int32 w, h, max_level, n, max_count; float64 eps; float32 min_eig; uint8 prev [h][w], next [h][w]; float32 pts [n][2]
// out: float32 next [n][2]; float32 err [n]; uint8 status [n]; then the compaction: int32 n_out; uint8 status [n]; int32 idx [n]
int main(int argc, char **argv)
{
    if (argc != 3)
        return 2;
    FILE *f = fopen(argv[1], "rb");
    int32_t hd[5];
    double eps;
    float min_eig;
    if (!f || fread(hd, sizeof(hd), 1, f) != 1 || fread(&eps, 8, 1, f) != 1 || fread(&min_eig, 4, 1, f) != 1)
        return 3;
    const int w = hd[0], h = hd[1], n = hd[3];
    std::vector<uint8_t> prev((size_t)w * h), next((size_t)w * h), st((size_t)n + 1), st2;
    std::vector<float> pts((size_t)2 * n + 2), out((size_t)2 * n + 2), err((size_t)n + 1), o0((size_t)2 * n + 2), o1((size_t)2 * n + 2);
    std::vector<int32_t> idx((size_t)n + 1, -1);
    if (fread(prev.data(), 1, prev.size(), f) != prev.size() || fread(next.data(), 1, next.size(), f) != next.size() ||
        fread(pts.data(), 8, (size_t)n, f) != (size_t)n)
        return 3;
    fclose(f);
    fe_track(prev.data(), next.data(), w, h, hd[2], pts.data(), n, hd[4], eps, min_eig, out.data(), st.data(), err.data(), 1, 0);
    st2 = st;
    const int32_t n_out = fe_compact(pts.data(), out.data(), st2.data(), n, o0.data(), o1.data(), idx.data(), 256);
    f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), 8, (size_t)n, f) != (size_t)n || fwrite(err.data(), 4, (size_t)n, f) != (size_t)n ||
        fwrite(st.data(), 1, (size_t)n, f) != (size_t)n || fwrite(&n_out, 4, 1, f) != 1 || fwrite(st2.data(), 1, (size_t)n, f) != (size_t)n ||
        fwrite(idx.data(), 4, (size_t)n, f) != (size_t)n)
        return 6;
    fclose(f);
    return 0;
}
#endif
