// flow_win_emu.cpp -- TEST ONLY.  The windowed two-image tracker (lk.hip: lk_flow_win_kernel<W>, W odd in 5 .. 19; 21 is
// lk_flow_kernel) on the CPU through the coroutine SIMT emulator, over flow_emu.cpp's harness: the same plan, the same exactly
// sized heap block per pyramid level (a load outside a level aborts under AddressSanitizer -- the masked lanes' and the err
// epilogue's included), pyr_pass_kernel over the two images, then the kernel of the window over the points.  Two forms, as
// there: a shared library for tests/test_flow_win_emulation.py and -- with -DFLOW_WIN_EMU_MAIN -- a stand-alone program for the
// sanitizer tier, which reads one case from a file and writes the results to another.  Not a product path.
#include "flow_emu.cpp"

namespace {

template <int W>
void run_win(unsigned n_blocks, const vo::PyrImage *imgs, const vo::Quad *pairs, const float2 *in, const int *npts, int cap, int n_frames, int fpg,
             int ppp, float2 *out, uint8_t *st, float *er, const vo::LkParams &prm)
{
    for (unsigned b = 0; b < n_blocks; b++)
        emu::run_block(64, b, 0, 0, [&] {
            if constexpr (W == 21)
                vo::lk_flow_kernel(imgs, pairs, in, npts, cap, n_frames, fpg, ppp, out, st, er, prm);
            else
                vo::lk_flow_win_kernel<W>(imgs, pairs, in, npts, cap, n_frames, fpg, ppp, out, st, er, prm);
        });
}

} // namespace

extern "C" {

// fe_track (flow_emu.cpp) with a window: the launcher's switch of lk.hip (launch_lk_flow_win), 21 -> lk_flow_kernel.  Returns the
// number of pyramid levels built, -1 for a window without a kernel.
int fw_track(const uint8_t *prev, const uint8_t *next, int w, int h, int max_level, const float *pts, int n, int win, int max_count, double eps,
             float min_eig, float *next_out, uint8_t *status, float *err, int n_frames, int frame)
{
    using namespace vo;
    if (win < 5 || win > 21 || win % 2 == 0)
        return -1;
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
    // lk_grid of lk.hip
    const int fpg = n_frames >= 8 ? 8 : n_frames >= 4 ? 4 : n_frames >= 2 ? 2 : 1;
    const int parts = 8 / fpg, ppp = (n + parts - 1) / parts, groups = (n_frames + fpg - 1) / fpg;
    const unsigned nb = (unsigned)(8 * groups * ppp);
    float *e = err ? er.data() : nullptr;
    switch (win) {
#define FW_CASE(W)                                                                                                              \
    case W:                                                                                                                     \
        run_win<W>(nb, d_imgs, pairs.data(), in.data(), npts.data(), cap, n_frames, fpg, ppp, out.data(), st.data(), e, prm);   \
        break;
        FW_CASE(5) FW_CASE(7) FW_CASE(9) FW_CASE(11) FW_CASE(13) FW_CASE(15) FW_CASE(17) FW_CASE(19) FW_CASE(21)
#undef FW_CASE
    }
    memcpy(next_out, &out[(size_t)frame * cap], sizeof(float2) * (size_t)n);
    memcpy(status, &st[(size_t)frame * cap], (size_t)n);
    if (err)
        memcpy(err, &er[(size_t)frame * cap], sizeof(float) * (size_t)n);
    return p.levels;
}
}

#ifdef FLOW_WIN_EMU_MAIN
#include <stdio.h>
// in:  int32 w, h, max_level, n, max_count, win; float64 eps; float32 min_eig; uint8 prev [h][w], next [h][w]; float32 pts [n][2]
// out: float32 next [n][2]; float32 err [n]; uint8 status [n]
int main(int argc, char **argv)
{
    if (argc != 3)
        return 2;
    FILE *f = fopen(argv[1], "rb");
    int32_t hd[6];
    double eps;
    float min_eig;
    if (!f || fread(hd, sizeof(hd), 1, f) != 1 || fread(&eps, 8, 1, f) != 1 || fread(&min_eig, 4, 1, f) != 1)
        return 3;
    const int w = hd[0], h = hd[1], n = hd[3];
    std::vector<uint8_t> prev((size_t)w * h), next((size_t)w * h), st((size_t)n + 1);
    std::vector<float> pts((size_t)2 * n + 2), out((size_t)2 * n + 2), err((size_t)n + 1);
    if (fread(prev.data(), 1, prev.size(), f) != prev.size() || fread(next.data(), 1, next.size(), f) != next.size() ||
        fread(pts.data(), 8, (size_t)n, f) != (size_t)n)
        return 3;
    fclose(f);
    if (fw_track(prev.data(), next.data(), w, h, hd[2], pts.data(), n, hd[5], hd[4], eps, min_eig, out.data(), st.data(), err.data(), 1, 0) < 0)
        return 4;
    f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), 8, (size_t)n, f) != (size_t)n || fwrite(err.data(), 4, (size_t)n, f) != (size_t)n ||
        fwrite(st.data(), 1, (size_t)n, f) != (size_t)n)
        return 6;
    fclose(f);
    return 0;
}
#endif
