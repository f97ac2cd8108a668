// emu_pyramid.h -- TEST ONLY.  The image table of the emulated runs (kernel_emu.cpp, flow_emu.cpp): the level plan of libvo_hip
// and a heap that holds it.  Include after the product sources (vo_kernels.h: plan_depth, level_stride).
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

} // namespace
