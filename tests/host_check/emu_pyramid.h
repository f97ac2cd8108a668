// emu_pyramid.h -- TEST ONLY.  What the emulated LK runs share (kernel_emu.cpp, chain_emu.cpp, flow_emu.cpp): the level plan of
// libvo_hip and a heap that holds it, the fused pyramid passes over that heap, the tracker's parameters and the arrays of a batch
// of frames.  Include after hip_emu.h and the product sources (lk.hip, pyramid.hip).
#pragma once

#include <memory>
#include <vector>

namespace {

// the geometry libvo_hip plans (capi.hip: plan_levels)
struct Plan {
    int levels = 0;
    int lw[VO_MAX_LEVELS], lh[VO_MAX_LEVELS], ls[VO_MAX_LEVELS];
};

Plan plan(int w, int h, int max_level)
{
    Plan p;
    p.levels = vo::plan_depth(w, h, max_level) + 1;
    for (int l = 0; l < p.levels; l++, w = (w + 1) / 2, h = (h + 1) / 2) {
        p.lw[l] = w;
        p.lh[l] = h;
        p.ls[l] = vo::level_stride(w);
    }
    return p;
}

// Every level of every image in its OWN heap block of exactly ls * (lh + 2 VO_BY) bytes / dwords.  That is tighter than the
// product's table (capi.hip: levels one after the other at 256-byte boundaries, the images one after the other, vo_create's
// worst-case slack behind the last): under AddressSanitizer any kernel access outside a level's bordered allocation aborts,
// whichever level, image or pyramid depth it belongs to.  Pixels are poisoned with 0xA5 (a read of border the build did not
// write shows up), derivatives zero.  imgs: n_img tight w x h images.
struct Heap {
    Plan p;
    std::vector<std::unique_ptr<uint8_t[]>> pix;
    std::vector<std::unique_ptr<uint32_t[]>> der;
    std::vector<vo::PyrImage> tab;
    size_t level_elems(int l) const { return (size_t)p.ls[l] * (p.lh[l] + 2 * VO_BY); }
    uint8_t *pix_block(int i, int l) { return pix[(size_t)i * p.levels + l].get(); }
    uint32_t *der_block(int i, int l) { return der[(size_t)i * p.levels + l].get(); }
    Heap(const Plan &plan_, const uint8_t *const *imgs, int n_img, int w, int h) : p(plan_), tab((size_t)n_img)
    {
        for (int i = 0; i < n_img; i++) {
            memset(&tab[i], 0, sizeof(vo::PyrImage));
            for (int l = 0; l < p.levels; l++) {
                const size_t n = level_elems(l), org = (size_t)VO_BY * p.ls[l] + VO_BX;
                pix.emplace_back(new uint8_t[n]);
                der.emplace_back(new uint32_t[n]);
                memset(pix.back().get(), 0xA5, n);
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

// the fused passes over every image of the heap, one launch per level (what launch_pyramid_fused enqueues).  remap 0: workgroups in
// dispatch order and thin border items, what launches of fewer than 16 images use; 1: the XCD-aware order with wide items
void build_fused_pyramids(Heap &heap, int n_img, int remap = 0)
{
    using namespace vo;
    const Plan &p = heap.p;
    const PyrImage *d_imgs = heap.tab.data();
    const PassPlan pp = pass_plan(p.levels, p.lw, p.lh, p.ls, /*wide border items*/ remap != 0);
    for (int l = 0; l < p.levels; l++) {
        const uint32_t nwg = pass_grid(pp, l, n_img, remap);
        for (uint32_t b = 0; b < nwg; b++)
            emu::run_block(64, b, 0, 0, [&] { pyr_pass_kernel(d_imgs, l, p.levels, pp, (uint32_t)n_img, remap); });
    }
}

// the tracker's parameters over every level of the plan: the reference's 30 / 0.01 / 1e-3 unless the caller has its own
vo::LkParams lk_params(const Plan &p, int full_chain, int max_count = 30, double eps = 0.01, float min_eig = 1e-3f)
{
    vo::LkParams prm;
    prm.max_level = p.levels - 1;
    prm.max_count = max_count;
    prm.epsilon = eps * eps;
    prm.min_eig = min_eig;
    prm.full_chain = full_chain;
    return prm;
}

// The arrays of one launch over n_frames frames of `hops` hops each.  quads [n_frames][4]: indices (l0, r0, l1, r1) into the image
// table, null: the pair (0, 1, 1, 0) in every frame.  pts: frame f's n points at pts + f * pts_stride floats.  Frame f tracks its
// first counts[f] points, clamped to 0 .. n (null: n in every frame); most: the largest count.  The frame stride of the device
// arrays is cap = n + 3, not n.  The outputs start as garbage (123456, -7 / 0xA5): rows a kernel must not write come back as that.
struct ChainBatch {
    int n_frames, n, hops, cap, most;
    std::vector<vo::Quad> q;
    std::vector<int> npts;
    std::vector<float2> in, out;
    std::vector<uint8_t> st;
    ChainBatch(const int *quads, int n_frames_, const float *pts, size_t pts_stride, const int *counts, int n_, int hops_)
        : n_frames(n_frames_), n(n_), hops(hops_), cap(n_ + 3), most(counts ? 0 : n_), q((size_t)n_frames_, vo::Quad{0, 1, 1, 0}),
          npts((size_t)n_frames_, n_), in((size_t)n_frames_ * cap), out((size_t)n_frames_ * hops_ * cap, make_float2(123456.f, -7.f)),
          st((size_t)n_frames_ * hops_ * cap, (uint8_t)0xA5)
    {
        for (int f = 0; f < n_frames; f++) {
            if (quads)
                q[(size_t)f] = vo::Quad{quads[4 * f], quads[4 * f + 1], quads[4 * f + 2], quads[4 * f + 3]};
            if (counts) {
                npts[(size_t)f] = counts[f] < 0 ? 0 : counts[f] > n ? n : counts[f];
                most = npts[(size_t)f] > most ? npts[(size_t)f] : most;
            }
            memcpy(&in[(size_t)f * cap], pts + (size_t)f * pts_stride, sizeof(float2) * (size_t)n);
        }
    }
    // to the caller's tight trk [n_frames][hops][n][2] and status [n_frames][hops][n]
    void copy_back(float *trk, uint8_t *status) const
    {
        for (int r = 0; r < n_frames * hops; r++) {
            memcpy(trk + (size_t)r * 2 * n, &out[(size_t)r * cap], sizeof(float2) * (size_t)n);
            memcpy(status + (size_t)r * n, &st[(size_t)r * cap], (size_t)n);
        }
    }
};

} // namespace
