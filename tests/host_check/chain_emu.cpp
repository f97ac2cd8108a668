// chain_emu.cpp -- TEST ONLY.  The 4-hop chain kernels of lk.hip (lk_circular_kernel, lk_hops_kernel, lk_circular_queue_kernel) over a
// BATCH of frames on the CPU, through the coroutine SIMT emulator of hip_emu.h: pyr_pass_kernel (pyramid.hip) over an image table,
// then the chain over the product's lk_grid -- the frame -> XCD numbering with parts of a frame's list (fewer than 8 frames) and a
// partial last group included, which kernel_emu.cpp's one-frame launch does not reach -- or, for the queue kernel, over its
// lk_queue_grid in a chosen order of the workgroups (cq_chain).  Every level of every pyramid is a heap block of its own of exactly
// stride x (h + 2 VO_BY) bytes / dwords (emu_pyramid.h): under AddressSanitizer a tile fill or a template read outside a level
// aborts.  Two forms: a shared library for tests/lk_chain_cases.py and tests/lk_queue_cases.py and -- with -DCHAIN_EMU_MAIN -- a
// stand-alone program (built with -fsanitize=address,undefined and run as a child; nothing instrumented is loaded into python).
// Not a product path.
#include "hip_emu.h"

#include "../../visual_odom_amd/csrc/lk.hip"
#include "../../visual_odom_amd/csrc/pyramid.hip"

#include "emu_pyramid.h"

namespace {

// the pyramids of n_img tight w x h images, each level in its heap block, built by the fused passes
Heap pyramids(const uint8_t *imgs, int n_img, int w, int h, int max_level)
{
    std::vector<const uint8_t *> img_ptr;
    for (int i = 0; i < n_img; i++)
        img_ptr.push_back(imgs + (size_t)i * w * h);
    Heap heap(plan(w, h, max_level), img_ptr.data(), n_img, w, h);
    build_fused_pyramids(heap, n_img);
    return heap;
}

} // namespace

extern "C" {

// imgs: n_img tight w x h gray images; quads [n_frames][4]: indices (l0, r0, l1, r1) into them; pts [n_frames][n][2], frame f
// tracks its first counts[f]; split: 0 = one launch of lk_circular_kernel, 1 = lk_hops_kernel [0, 1) + [1, 4) over outputs that
// start as garbage.  trk [n_frames][4][n][2], status [n_frames][4][n]; rows from counts[f] on come back untouched (123456, -7 /
// 0xA5).  Returns the number of pyramid levels built.
int ce_chain(const uint8_t *imgs, int n_img, int w, int h, int max_level, const int *quads, int n_frames, const float *pts, const int *counts,
             int n, int full_chain, int split, float *trk, uint8_t *status)
{
    using namespace vo;
    Heap heap = pyramids(imgs, n_img, w, h, max_level);
    const PyrImage *d_imgs = heap.tab.data();
    const LkParams prm = lk_params(heap.p, full_chain);
    ChainBatch bt(quads, n_frames, pts, (size_t)2 * n, counts, n, 4);
    if (bt.most > 0) {
        const LkGrid g = lk_grid(n_frames, bt.most);
        const int cut[3] = {0, split ? 1 : 4, 4};
        for (int k = 0; k < (split ? 2 : 1); k++)
            for (int b = 0; b < g.blocks; b++)
                emu::run_block(64, (unsigned)b, 0, 0, [&] {
                    if (split)
                        lk_hops_kernel(d_imgs, bt.q.data(), bt.in.data(), bt.npts.data(), bt.cap, n_frames, g.fpg, g.ppp, bt.out.data(), bt.st.data(),
                                       prm, cut[k], cut[k + 1]);
                    else
                        lk_circular_kernel(d_imgs, bt.q.data(), bt.in.data(), bt.npts.data(), bt.cap, n_frames, g.fpg, g.ppp, bt.out.data(),
                                           bt.st.data(), prm);
                });
    }
    bt.copy_back(trk, status);
    return heap.p.levels;
}

// lk_circular_queue_kernel (the work item drawn from the per-XCD ticket queues of vo_lkqueue.h) against lk_circular_kernel over one
// batch.  The emulator runs one workgroup at a time, so the ORDER in which the workgroups are run is the order in which they draw:
// dispatch order, reverse order, and all workgroups of one XCD before any other (its surplus workgroups then take the next queue's
// first tickets).  The arguments of ce_chain, and
//   order: -1 = lk_circular_kernel over lk_grid; 0 / 1 / 2 = lk_circular_queue_kernel over lk_queue_grid(surplus_div) with the
//          workgroups in dispatch order / in reverse / those of XCD first_xcd first, then the rest in dispatch order
//   stats [5] (order >= 0): workgroups, workgroups that found every queue dry, workgroups whose item came from another XCD's
//          queue, the largest number of draws of one workgroup, workgroups that drew once and found their XCD marked all dry
// The launch draws from counter set 0 and finds set 1 filled with garbage.  Returns the number of pyramid levels built, or a
// negative number: -1 a counter of the drawn set ends below its queue's length, -2 the other set is not zero afterwards, -3 a
// workgroup on a marked XCD drew more than once or got an item, or one that found every queue dry left no mark.
int cq_chain(const uint8_t *imgs, int n_img, int w, int h, int max_level, const int *quads, int n_frames, const float *pts, const int *counts,
             int n, int full_chain, int order, int first_xcd, int surplus_div, float *trk, uint8_t *status, int *stats)
{
    using namespace vo;
    if (order < 0)
        return ce_chain(imgs, n_img, w, h, max_level, quads, n_frames, pts, counts, n, full_chain, 0, trk, status);
    Heap heap = pyramids(imgs, n_img, w, h, max_level);
    const PyrImage *d_imgs = heap.tab.data();
    const LkParams prm = lk_params(heap.p, full_chain);
    ChainBatch bt(quads, n_frames, pts, (size_t)2 * n, counts, n, 4);
    int rc = heap.p.levels;
    if (bt.most > 0) {
        const LkQueueGrid g = lk_queue_grid(n_frames, bt.most, surplus_div);
        std::vector<unsigned> ctr((size_t)LKQ_WORDS, 0u);
        unsigned *const cur = ctr.data(), *const oth = ctr.data() + LKQ_QUEUES * LKQ_STRIDE;
        for (int i = 0; i < LKQ_QUEUES; i++)
            oth[LKQ_STRIDE * i] = 0xDEAD0000u + (unsigned)i;
        std::vector<int> run;
        for (int b = 0; b < g.blocks; b++)
            if (order == 2 && (b & 7) == first_xcd)
                run.push_back(b);
        for (int b = 0; b < g.blocks; b++)
            if (!(order == 2 && (b & 7) == first_xcd))
                run.push_back(order == 1 ? g.blocks - 1 - b : b);
        stats[0] = g.blocks;
        stats[1] = stats[2] = stats[3] = stats[4] = 0;
        for (int b : run) {
            unsigned before[LKQ_QUEUES], draws = 0;
            for (int i = 0; i < LKQ_QUEUES; i++)
                before[i] = cur[LKQ_STRIDE * i] & ~LKQ_ALL_DRY;
            const bool marked = (cur[LKQ_STRIDE * (b & 7)] & LKQ_ALL_DRY) != 0;
            emu::run_block(64, (unsigned)b, 0, 0, [&] {
                lk_circular_queue_kernel(d_imgs, bt.q.data(), bt.in.data(), bt.npts.data(), bt.cap, n_frames, g.fpg, g.ppp, bt.out.data(),
                                         bt.st.data(), prm, g.items, cur, oth);
            });
            int last = -1;
            for (int k = 0; k < LKQ_QUEUES; k++) { // (the queues in the order this workgroup visits them)
                const int i = ((b & 7) + k) & 7;
                const unsigned d = (cur[LKQ_STRIDE * i] & ~LKQ_ALL_DRY) - before[i];
                draws += d;
                if (d)
                    last = i;
            }
            const bool dry = last < 0 || before[last] >= (unsigned)g.items;
            stats[1] += dry;
            stats[4] += marked;
            if (marked && (draws != 1 || !dry)) // (a marked XCD: one draw, no item)
                rc = -3;
            if (dry && !(cur[LKQ_STRIDE * (b & 7)] & LKQ_ALL_DRY)) // (whoever finds all dry leaves the mark)
                rc = -3;
            stats[2] += !dry && last != (b & 7);
            stats[3] = (int)draws > stats[3] ? (int)draws : stats[3];
        }
        for (int i = 0; i < LKQ_QUEUES; i++) {
            if ((cur[LKQ_STRIDE * i] & ~LKQ_ALL_DRY) < (unsigned)g.items)
                rc = -1;
            if (oth[LKQ_STRIDE * i] != 0u)
                rc = -2;
        }
    }
    bt.copy_back(trk, status);
    return rc;
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
