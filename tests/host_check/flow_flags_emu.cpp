// flow_flags_emu.cpp -- TEST ONLY.  The two-image tracker with flags (lk.hip: lk_flow_flags_kernel<W>, every odd W of 5 .. 21) on
// the CPU through the coroutine SIMT emulator, over flow_emu.cpp's harness like flow_win_emu.cpp: the same plan, the same exactly
// sized heap block per pyramid level (a load outside a level aborts under AddressSanitizer -- a far-off start's tile included),
// pyr_pass_kernel over the two images, then the launcher's route of lk.hip (launch_lk_flow_flags): flags 0 -> the kernel of the
// flags-less call, anything else lk_flow_flags_kernel<W> with the next-position rows in/out.  Frames of one launch may hold
// different point counts.  Two forms, as there: a shared library for tests/test_flow_flags_emulation.py and -- with
// -DFLOW_FLAGS_EMU_MAIN -- a stand-alone program for the sanitizer tier.  Not a product path.
#include "flow_emu.cpp"

namespace {

template <int W>
void run_flags(unsigned n_blocks, int flags, const vo::PyrImage *imgs, const vo::Quad *pairs, const float2 *in, const int *npts, int cap,
               int n_frames, int fpg, int ppp, float2 *out, uint8_t *st, float *er, const vo::LkParams &prm)
{
    for (unsigned b = 0; b < n_blocks; b++)
        emu::run_block(64, b, 0, 0, [&] {
            if (flags != 0)
                vo::lk_flow_flags_kernel<W>(imgs, pairs, in, npts, cap, n_frames, fpg, ppp, out, st, er, prm, flags);
            else if constexpr (W == 21)
                vo::lk_flow_kernel(imgs, pairs, in, npts, cap, n_frames, fpg, ppp, out, st, er, prm);
            else
                vo::lk_flow_win_kernel<W>(imgs, pairs, in, npts, cap, n_frames, fpg, ppp, out, st, er, prm);
        });
}

} // namespace

extern "C" {

// n_frames frames of the pair (prev, next) in one launch; frame f tracks the first counts[f] of the n points (counts == null: n in
// every frame).  next_io [n_frames][n][2]: the guesses in (read with flags & 4 only), the results out; status [n_frames][n]; err
// [n_frames][n] or null.  Rows from counts[f] on come back as the kernel left them: untouched (guesses / 0xA5 / -1).  Returns the
// number of pyramid levels built, -1 for a window or flags without a kernel.
int ff_track(const uint8_t *prev, const uint8_t *next, int w, int h, int max_level, const float *pts, int n, int win, int flags, int max_count,
             double eps, float min_eig, float *next_io, uint8_t *status, float *err, int n_frames, const int *counts)
{
    using namespace vo;
    if (win < 5 || win > 21 || win % 2 == 0 || (flags & ~(VO_LK_USE_INITIAL_FLOW | VO_LK_GET_MIN_EIGENVALS)) || n_frames < 1)
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
    int most = counts ? 0 : n;
    for (int f = 0; counts && f < n_frames; f++) {
        npts[(size_t)f] = counts[f] < 0 ? 0 : counts[f] > n ? n : counts[f];
        most = npts[(size_t)f] > most ? npts[(size_t)f] : most;
    }
    std::vector<float2> in((size_t)n_frames * cap), out((size_t)n_frames * cap, make_float2(123456.f, -7.f));
    std::vector<uint8_t> st((size_t)n_frames * cap, (uint8_t)0xA5);
    std::vector<float> er((size_t)n_frames * cap, -1.f);
    for (int f = 0; f < n_frames; f++) {
        memcpy(&in[(size_t)f * cap], pts, sizeof(float2) * (size_t)n);
        if (flags & VO_LK_USE_INITIAL_FLOW)
            memcpy(&out[(size_t)f * cap], next_io + (size_t)f * 2 * n, sizeof(float2) * (size_t)n);
    }
    if (most > 0) {
        // lk_grid of lk.hip over the largest count (the library's max_pts)
        const int fpg = n_frames >= 8 ? 8 : n_frames >= 4 ? 4 : n_frames >= 2 ? 2 : 1;
        const int parts = 8 / fpg, ppp = (most + parts - 1) / parts, groups = (n_frames + fpg - 1) / fpg;
        const unsigned nb = (unsigned)(8 * groups * ppp);
        float *e = err ? er.data() : nullptr;
        switch (win) {
#define FF_CASE(W)                                                                                                              \
    case W:                                                                                                                     \
        run_flags<W>(nb, flags, d_imgs, pairs.data(), in.data(), npts.data(), cap, n_frames, fpg, ppp, out.data(), st.data(), e, prm); \
        break;
            FF_CASE(5) FF_CASE(7) FF_CASE(9) FF_CASE(11) FF_CASE(13) FF_CASE(15) FF_CASE(17) FF_CASE(19) FF_CASE(21)
#undef FF_CASE
        }
    }
    for (int f = 0; f < n_frames; f++) {
        memcpy(next_io + (size_t)f * 2 * n, &out[(size_t)f * cap], sizeof(float2) * (size_t)n);
        memcpy(status + (size_t)f * n, &st[(size_t)f * cap], (size_t)n);
        if (err)
            memcpy(err + (size_t)f * n, &er[(size_t)f * cap], sizeof(float) * (size_t)n);
    }
    return p.levels;
}
}

#ifdef FLOW_FLAGS_EMU_MAIN
#include <stdio.h>
// in:  int32 w, h, max_level, n, max_count, win, flags; float64 eps; float32 min_eig; uint8 prev [h][w], next [h][w];
//      float32 pts [n][2], guess [n][2]
// out: float32 next [n][2]; float32 err [n]; uint8 status [n]
int main(int argc, char **argv)
{
    if (argc != 3)
        return 2;
    FILE *f = fopen(argv[1], "rb");
    int32_t hd[7];
    double eps;
    float min_eig;
    if (!f || fread(hd, sizeof(hd), 1, f) != 1 || fread(&eps, 8, 1, f) != 1 || fread(&min_eig, 4, 1, f) != 1)
        return 3;
    const int w = hd[0], h = hd[1], n = hd[3];
    std::vector<uint8_t> prev((size_t)w * h), next((size_t)w * h), st((size_t)n + 1);
    std::vector<float> pts((size_t)2 * n + 2), io((size_t)2 * n + 2), err((size_t)n + 1);
    if (fread(prev.data(), 1, prev.size(), f) != prev.size() || fread(next.data(), 1, next.size(), f) != next.size() ||
        fread(pts.data(), 8, (size_t)n, f) != (size_t)n || fread(io.data(), 8, (size_t)n, f) != (size_t)n)
        return 3;
    fclose(f);
    if (ff_track(prev.data(), next.data(), w, h, hd[2], pts.data(), n, hd[5], hd[6], hd[4], eps, min_eig, io.data(), st.data(), err.data(), 1,
                 nullptr) < 0)
        return 4;
    f = fopen(argv[2], "wb");
    if (!f || fwrite(io.data(), 8, (size_t)n, f) != (size_t)n || fwrite(err.data(), 4, (size_t)n, f) != (size_t)n ||
        fwrite(st.data(), 1, (size_t)n, f) != (size_t)n)
        return 6;
    fclose(f);
    return 0;
}
#endif
