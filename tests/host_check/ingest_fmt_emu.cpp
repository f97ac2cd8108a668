// ingest_fmt_emu.cpp -- TEST ONLY.  Executes the product's converting ingest kernels (visual_odom_amd/csrc/ingest_fmt.hip) on
// the CPU through the coroutine SIMT emulator of hip_emu.h.  Every SOURCE image is copied into a heap block of its own of
// exactly the bytes the format's contract allows a kernel to read -- (h - 1) * stride + w * bpp, for one plane of a two-byte
// interleave (h - 1) * stride + 2 w - 1 -- so that under AddressSanitizer (VO_SANITIZE=1) any over-read aborts.  Not a product path.
#include "hip_emu.h"

#include "../../visual_odom_amd/csrc/ingest_fmt.hip"

#include <memory>
#include <vector>

namespace {

template <typename F>
void launch(unsigned gx, int threads, F body)
{
    for (unsigned x = 0; x < gx; x++)
        emu::run_block(threads, x, 0, 0, body);
}

std::unique_ptr<uint8_t[]> tight(const uint8_t *src, size_t n)
{
    std::unique_ptr<uint8_t[]> p(new uint8_t[n]);
    memcpy(p.get(), src, n);
    return p;
}

template <int FMT>
void seq_go(const vo::SeqIngest *tab, int n_rows, int n_waves, int w, int h, int pitch, uint8_t *dst)
{
    launch((unsigned)n_waves, 64, [&] { vo::seq_ingest_fmt_kernel<FMT>(tab, n_rows, n_waves, w, h, pitch, dst, (size_t)h * pitch); });
}

template <int FMT>
void pull_go(const uint8_t *src, int stride, uint8_t *dst, int pitch, int w, int h, const uint2 *src2, uint2 *dst2, uint32_t n8, int *count_dst,
             int count)
{
    const uint32_t waves = (uint32_t)h * (uint32_t)((w + 511) / 512), img_blocks = (waves + 3) / 4; // (launch_pull_image_fmt's grid)
    launch(img_blocks + (n8 + 255) / 256, 256, [&] { vo::pull_image_fmt_kernel<FMT>(src, stride, dst, pitch, w, h, img_blocks, src2, dst2, n8, count_dst, count); });
}

} // namespace

extern "C" {

// seq_ingest_fmt_kernel<fmt>: n_pairs pairs of w x h images with a byte stride -> pitched gray images (pair i: images 2 i,
// 2 i + 1) by n_waves single-wave workgroups.  right == NULL: every left[i] is an INTERLEAVED buffer of (h - 1) * stride + 2 w
// bytes and the pair is (buf, buf + 1), the read-once form; otherwise left[i] / right[i] hold src_bytes bytes each.
int ife_seq_ingest(int fmt, const uint8_t *const *left, const uint8_t *const *right, size_t src_bytes, int n_pairs, int w, int h, int stride,
                   int pitch, uint8_t *dst /* [2 n_pairs][h][pitch] */, int n_waves)
{
    using namespace vo;
    std::vector<std::unique_ptr<uint8_t[]>> keep;
    std::vector<SeqIngest> tab((size_t)n_pairs);
    for (int i = 0; i < n_pairs; i++) {
        keep.push_back(tight(left[i], src_bytes));
        tab[i].left = keep.back().get();
        if (right) {
            keep.push_back(tight(right[i], src_bytes));
            tab[i].right = keep.back().get();
        } else {
            tab[i].right = tab[i].left + 1;
        }
        tab[i].stride = stride;
        tab[i].image0 = 2 * i;
    }
    const int n_rows = 2 * n_pairs * h;
    return ingest_dispatch(fmt, [&](auto tag) { seq_go<decltype(tag)::value>(tab.data(), n_rows, n_waves, w, h, pitch, dst); });
}

// pull_image_fmt_kernel<fmt>: one image of src_bytes bytes -> gray rows at `pitch`; n_pts float2 ride along (pts_src -> pts_dst) with their count
int ife_pull(int fmt, const uint8_t *src, size_t src_bytes, int stride, uint8_t *dst, int pitch, int w, int h, const float *pts_src, float *pts_dst,
             int n_pts, int *count_dst)
{
    using namespace vo;
    const std::unique_ptr<uint8_t[]> s = tight(src, src_bytes);
    const uint2 *p2 = (const uint2 *)pts_src;
    uint2 *d2 = (uint2 *)pts_dst;
    const uint32_t n8 = pts_dst ? (uint32_t)n_pts : 0u;
    return ingest_dispatch(fmt, [&](auto tag) { pull_go<decltype(tag)::value>(s.get(), stride, dst, pitch, w, h, p2, d2, n8, count_dst, n_pts); });
}

int ife_bpp(int fmt) { return vo::ingest_bpp(fmt); }
}
