// flow_emu.cpp -- TEST ONLY.  Executes the product's two-image tracker on the CPU through the coroutine SIMT emulator of hip_emu.h:
// pyr_pass_kernel (pyramid.hip) over the two images, the LK kernel of a window and flags (lk.hip: lk_flow_kernel,
// lk_flow_win_kernel<W>, lk_flow_flags_kernel<W>, picked by the product's own lk_for_window / lk_flow_route and launched over the
// product's lk_grid) over the points, flow_compact_kernel (post.hip) over the result.  Every level of both pyramids is a heap block
// of its own of exactly stride x (h + 2 VO_BY) bytes / dwords (emu_pyramid.h), so that under AddressSanitizer a load outside a
// level aborts -- the masked lanes', the err epilogue's tile refill and a far-off start's tile included.  Two forms: a shared
// library for tests/flow_emu.py, and -- with -DFLOW_EMU_MAIN -- a stand-alone program (the sanitizer tier: built with
// -fsanitize=address,undefined and run as a child, nothing instrumented is loaded into python) that reads one case from a file
// and writes the results to another.  Not a product path.
#include "hip_emu.h"

#include "../../visual_odom_amd/csrc/lk.hip"
#include "../../visual_odom_amd/csrc/pyramid.hip"
#include "../../visual_odom_amd/csrc/post.hip"

#include "emu_pyramid.h"

extern "C" {

// prev, next: tight w x h gray images; pts [n][2].  n_frames frames of the pair in one launch (the frame -> XCD numbering); frame
// f tracks the first counts[f] of the n points (counts == null: n in every frame).  next_io [n_frames][n][2]: the guesses in (read
// with flags & 4 only), the results out; status [n_frames][n]; err [n_frames][n] or null (the kernel's "not requested").  Rows
// from counts[f] on come back as the kernel left them: untouched (guesses / 0xA5 / -1).  Returns the number of pyramid levels
// built, -1 for a window or flags without a kernel.
int fe_track(const uint8_t *prev, const uint8_t *next, int w, int h, int max_level, const float *pts, int n, int win, int flags, int max_count,
             double eps, float min_eig, float *next_io, uint8_t *status, float *err, int n_frames, const int *counts)
{
    using namespace vo;
    if (!lk_for_window(win, [](auto) {}) || (flags & ~(VO_LK_USE_INITIAL_FLOW | VO_LK_GET_MIN_EIGENVALS)) || n_frames < 1)
        return -1;
    const uint8_t *imgs[2] = {prev, next};
    Heap heap(plan(w, h, max_level), imgs, 2, w, h);
    const PyrImage *d_imgs = heap.tab.data();
    build_fused_pyramids(heap, 2);
    if (n <= 0)
        return heap.p.levels;
    const LkParams prm = lk_params(heap.p, /*full_chain*/ 0, max_count, eps, min_eig);
    ChainBatch bt(nullptr, n_frames, pts, 0, counts, n, 1); // (the pair and the points of every frame are the call's)
    std::vector<float> er((size_t)n_frames * bt.cap, -1.f);
    if (flags & VO_LK_USE_INITIAL_FLOW)
        for (int f = 0; f < n_frames; f++)
            memcpy(&bt.out[(size_t)f * bt.cap], next_io + (size_t)f * 2 * n, sizeof(float2) * (size_t)n);
    if (bt.most > 0) { // launch_lk_flow of lk.hip over the largest count (the library's max_pts), a loop over the blocks as the launch
        const LkGrid g = lk_grid(n_frames, bt.most);
        lk_for_window(win, [&](auto wc) {
            lk_flow_route<decltype(wc)::value>(flags, [&](auto kernel, auto... tail) {
                for (int b = 0; b < g.blocks; b++)
                    emu::run_block(64, (unsigned)b, 0, 0, [&] {
                        kernel(d_imgs, bt.q.data(), bt.in.data(), bt.npts.data(), bt.cap, n_frames, g.fpg, g.ppp, bt.out.data(), bt.st.data(),
                               err ? er.data() : nullptr, prm, tail...);
                    });
            });
        });
    }
    bt.copy_back(next_io, status);
    for (int f = 0; err && f < n_frames; f++)
        memcpy(err + (size_t)f * n, &er[(size_t)f * bt.cap], sizeof(float) * (size_t)n);
    return heap.p.levels;
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
// in:  int32 w, h, max_level, n, max_count, win, flags; float64 eps; float32 min_eig; uint8 prev [h][w], next [h][w];
//      float32 pts [n][2], guess [n][2]
// out: float32 next [n][2]; float32 err [n]; uint8 status [n]; then the compaction: int32 n_out; uint8 status [n]; int32 idx [n]
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
    std::vector<uint8_t> prev((size_t)w * h), next((size_t)w * h), st((size_t)n + 1), st2;
    std::vector<float> pts((size_t)2 * n + 2), io((size_t)2 * n + 2), err((size_t)n + 1), o0((size_t)2 * n + 2), o1((size_t)2 * n + 2);
    std::vector<int32_t> idx((size_t)n + 1, -1);
    if (fread(prev.data(), 1, prev.size(), f) != prev.size() || fread(next.data(), 1, next.size(), f) != next.size() ||
        fread(pts.data(), 8, (size_t)n, f) != (size_t)n || fread(io.data(), 8, (size_t)n, f) != (size_t)n)
        return 3;
    fclose(f);
    if (fe_track(prev.data(), next.data(), w, h, hd[2], pts.data(), n, hd[5], hd[6], hd[4], eps, min_eig, io.data(), st.data(), err.data(), 1,
                 nullptr) < 0)
        return 4;
    st2 = st;
    const int32_t n_out = fe_compact(pts.data(), io.data(), st2.data(), n, o0.data(), o1.data(), idx.data(), 256);
    f = fopen(argv[2], "wb");
    if (!f || fwrite(io.data(), 8, (size_t)n, f) != (size_t)n || fwrite(err.data(), 4, (size_t)n, f) != (size_t)n ||
        fwrite(st.data(), 1, (size_t)n, f) != (size_t)n || fwrite(&n_out, 4, 1, f) != 1 || fwrite(st2.data(), 1, (size_t)n, f) != (size_t)n ||
        fwrite(idx.data(), 4, (size_t)n, f) != (size_t)n)
        return 6;
    fclose(f);
    return 0;
}
#endif
