// rectify_emu.cpp -- TEST ONLY.  Executes the product's rectify_kernel (visual_odom_amd/csrc/rectify.hip) on the CPU through the
// coroutine SIMT emulator of hip_emu.h, behind the product's own host packing (vo_rectify.h: rect_pack).  Every RAW PLANE is a
// heap block of its own of exactly rect_raw_bytes(w, h) -- zero frame, interior copied in -- and so are the packed maps, so that
// under AddressSanitizer a tap or a map load outside them aborts.  Two forms: a shared library for tests/test_rectify_emulation.py,
// and -- with -DRECTIFY_EMU_MAIN -- a stand-alone program (the sanitizer tier: built with -fsanitize=address,undefined and run as
// a child, nothing instrumented is loaded into python) that reads one case from a file and writes the destination images to
// another.  Not a product path.
#include "hip_emu.h"

#include "../../visual_odom_amd/csrc/rectify.hip"

#include <memory>
#include <vector>

extern "C" {

// the product's packing of one side's maps (rows stride_floats apart) -> w * h dwords; 0, or -1: a displacement out of range
int rfe_pack(const float *mx, const float *my, int stride_floats, int w, int h, uint32_t *out)
{
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++)
            if (!vo::rect_pack(mx[(size_t)y * stride_floats + x], my[(size_t)y * stride_floats + x], x, y, w, h, &out[(size_t)y * w + x]))
                return -1;
    return 0;
}

// rectify_kernel over n tight w x h gray images (src[i], side sides[i]) -> image i of dst [n][h][pitch], by n_waves single-wave
// workgroups; packed: the left side's w * h dwords, then the right side's
int rfe_rectify(const uint8_t *const *src, const int *sides, int n, int w, int h, const uint32_t *packed, int pitch, uint8_t *dst, int n_waves)
{
    using namespace vo;
    const int rp = rect_raw_pitch(w);
    std::vector<std::unique_ptr<uint8_t[]>> planes;
    std::vector<RectImage> tab((size_t)n);
    for (int i = 0; i < n; i++) {
        planes.emplace_back(new uint8_t[rect_raw_bytes(w, h)]());
        uint8_t *p0 = planes.back().get() + rect_raw_origin(w);
        for (int y = 0; y < h; y++)
            memcpy(p0 + (size_t)y * rp, src[i] + (size_t)y * w, (size_t)w);
        tab[i] = RectImage{p0, i, sides[i]};
    }
    std::unique_ptr<uint32_t[]> maps(new uint32_t[(size_t)2 * w * h]);
    memcpy(maps.get(), packed, sizeof(uint32_t) * 2 * w * h);
    const int n_items = n * h * ((w + 255) / 256);
    for (int b = 0; b < n_waves; b++)
        emu::run_block(64, (unsigned)b, 0, 0,
                       [&] { rectify_kernel(tab.data(), n_items, n_waves, w, h, rp, maps.get(), pitch, dst, (size_t)h * pitch); });
    return 0;
}

int rfe_raw_pitch(int w) { return vo::rect_raw_pitch(w); }
}

#ifdef RECTIFY_EMU_MAIN
#include <stdio.h>
// in:  int32 n, w, h, pitch, n_waves, guard; int32 sides[n]; float map_x_left, map_y_left, map_x_right, map_y_right [h][w];
//      uint8 images [n][h][w]
// out: uint8 [n][h][pitch], bytes outside the w columns = guard
int main(int argc, char **argv)
{
    if (argc != 3)
        return 2;
    FILE *f = fopen(argv[1], "rb");
    int32_t hd[6];
    if (!f || fread(hd, sizeof(hd), 1, f) != 1)
        return 3;
    const int n = hd[0], w = hd[1], h = hd[2], pitch = hd[3], n_waves = hd[4];
    const size_t px = (size_t)w * h;
    std::vector<int32_t> sides((size_t)n);
    std::vector<float> maps(4 * px);
    std::vector<uint8_t> imgs((size_t)n * px), dst((size_t)n * h * pitch, (uint8_t)hd[5]);
    if (fread(sides.data(), 4, (size_t)n, f) != (size_t)n || fread(maps.data(), 4, 4 * px, f) != 4 * px || fread(imgs.data(), 1, imgs.size(), f) != imgs.size())
        return 3;
    fclose(f);
    std::vector<uint32_t> packed(2 * px);
    for (int side = 0; side < 2; side++)
        if (rfe_pack(&maps[(size_t)(2 * side) * px], &maps[(size_t)(2 * side + 1) * px], w, w, h, &packed[(size_t)side * px]) != 0)
            return 4;
    std::vector<const uint8_t *> src((size_t)n);
    for (int i = 0; i < n; i++)
        src[i] = &imgs[(size_t)i * px];
    if (rfe_rectify(src.data(), sides.data(), n, w, h, packed.data(), pitch, dst.data(), n_waves) != 0)
        return 5;
    f = fopen(argv[2], "wb");
    if (!f || fwrite(dst.data(), 1, dst.size(), f) != dst.size())
        return 6;
    fclose(f);
    return 0;
}
#endif
