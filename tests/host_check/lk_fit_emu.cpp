// lk_fit_emu.cpp -- TEST ONLY.  The CPU-emulator harness of tests/lk_fit.py: flow_emu.cpp as it is (fe_track: the two-image kernels of
// every window), the 4-hop chain kernel over a batch (lf_chain: chain_emu.cpp's ce_chain without the split form), and the counter
// that lk.hip keeps under VO_HOST_EMUL only -- iterations per pyramid level with the split sums and with the 32-bit ones
// (wave_sum2_f32's two tails) -- so that a test can tell which path its images took.  One library, so one counter.  Not a product path.
#include "flow_emu.cpp"

extern "C" {

// the arguments of ce_chain (chain_emu.cpp) without `split`; returns the number of pyramid levels built
int lf_chain(const uint8_t *imgs, int n_img, int w, int h, int max_level, const int *quads, int n_frames, const float *pts, const int *counts,
             int n, int full_chain, float *trk, uint8_t *status)
{
    using namespace vo;
    std::vector<const uint8_t *> img_ptr;
    for (int i = 0; i < n_img; i++)
        img_ptr.push_back(imgs + (size_t)i * w * h);
    Heap heap(plan(w, h, max_level), img_ptr.data(), n_img, w, h);
    build_fused_pyramids(heap, n_img);
    const PyrImage *d_imgs = heap.tab.data();
    const LkParams prm = lk_params(heap.p, full_chain);
    ChainBatch bt(quads, n_frames, pts, (size_t)2 * n, counts, n, 4);
    if (bt.most > 0) {
        const LkGrid g = lk_grid(n_frames, bt.most);
        for (int b = 0; b < g.blocks; b++)
            emu::run_block(64, (unsigned)b, 0, 0, [&] {
                lk_circular_kernel(d_imgs, bt.q.data(), bt.in.data(), bt.npts.data(), bt.cap, n_frames, g.fpg, g.ppp, bt.out.data(), bt.st.data(), prm);
            });
    }
    bt.copy_back(trk, status);
    return heap.p.levels;
}

// out [VO_MAX_LEVELS][2]: iterations per level since the last reset, [0] split sums, [1] 32-bit sums
void lf_counts(long long *out, int reset)
{
    memcpy(out, vo::g_lk_fit_iterations, sizeof(vo::g_lk_fit_iterations));
    if (reset)
        memset(vo::g_lk_fit_iterations, 0, sizeof(vo::g_lk_fit_iterations));
}
}
