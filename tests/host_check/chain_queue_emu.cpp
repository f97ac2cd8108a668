// chain_queue_emu.cpp -- TEST ONLY.  lk_circular_queue_kernel (lk.hip: the work item drawn from the per-XCD ticket queues of
// vo_lkqueue.h) against lk_circular_kernel over one batch of frames on the CPU, through the coroutine SIMT emulator of hip_emu.h,
// the way chain_emu.cpp runs the chain: pyr_pass_kernel over the image table, then the chain.  The emulator runs one workgroup at
// a time, so the ORDER in which the workgroups are run is the order in which they draw: dispatch order, reverse order, and all
// workgroups of one XCD before any other (its surplus workgroups then take the next queue's first tickets).  Not a product path.
#include "hip_emu.h"

#include "../../visual_odom_amd/csrc/lk.hip"
#include "../../visual_odom_amd/csrc/pyramid.hip"

#include "emu_pyramid.h"

extern "C" {

// The arguments of chain_emu.cpp's ce_chain, and
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
    int rc = p.levels;
    if (most > 0 && order < 0) {
        const LkGrid g = lk_grid(n_frames, most);
        for (int b = 0; b < g.blocks; b++)
            emu::run_block(64, (unsigned)b, 0, 0, [&] {
                lk_circular_kernel(d_imgs, q.data(), in.data(), npts.data(), cap, n_frames, g.fpg, g.ppp, out.data(), st.data(), prm);
            });
    } else if (most > 0) {
        const LkQueueGrid g = lk_queue_grid(n_frames, most, surplus_div);
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
                lk_circular_queue_kernel(d_imgs, q.data(), in.data(), npts.data(), cap, n_frames, g.fpg, g.ppp, out.data(), st.data(), prm,
                                         g.items, cur, oth);
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
    for (int f = 0; f < n_frames; f++)
        for (int hop = 0; hop < 4; hop++) {
            memcpy(trk + ((size_t)f * 4 + hop) * 2 * n, &out[((size_t)f * 4 + hop) * cap], sizeof(float2) * (size_t)n);
            memcpy(status + ((size_t)f * 4 + hop) * n, &st[((size_t)f * 4 + hop) * cap], (size_t)n);
        }
    return rc;
}
}
