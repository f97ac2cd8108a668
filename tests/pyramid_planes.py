"""The one definition of what the bordered pyramid planes must hold, byte for byte (test_kernel_emulation.py::test_emulated_borders
and test_pyramid_planes.py on the CPU emulator, test_gpu_pyramid_planes.py on the MI355X through vo_batch_get_level_planes).

A level's planes are [rows][stride] with rows = h_l + 2 * BY and stride = BX + w_l + at least BY rounded up to 16, the image at
row BY, column BX:
  pix   the checker's build_pyramid level inside, cv::borderInterpolate(BORDER_REFLECT_101) of it everywhere else -- to the END of
        the row, and reflected repeatedly where a level is narrower or lower than the border;
  der   the checker's Scharr image * 4 packed as Ix | Iy << 16 inside, zero everywhere else (calcSharrDeriv's constant border).

Shapes (w, h): one level; second levels narrower / lower than the border on one axis each; three levels; four levels with the top
22 x 22 (repeated reflection on both axes); more than 64 column groups over a 23-row second level; 257 on either axis; and the
w mod 16 residues 9, 9, 15, 8 with every w mod 4.  Images: uniform noise (another seed per image of a batch, so a store into a
neighbouring image or level shows) and a 0 / 255 checkerboard (the extreme Scharr values of both signs)."""
import ctypes as C

import numpy as np

BX, BY = 32, 24
SHAPES = ((32, 32), (47, 45), (45, 47), (131, 97), (169, 169), (301, 45), (257, 64), (64, 257), (41, 60), (57, 33), (63, 39), (40, 40))
BIG = ((131, 97), (169, 169))        # the shapes that get every image count
COUNTS = (1, 4, 15, 16, 17, 24)      # last thin launch, first wide one, padding to a multiple of 8, a full third group
_CACHE = {}


def ids(shape):
    return "%dx%d" % shape


def stride(w):
    return (BX + w + BY + 15) // 16 * 16


def depth(w, h, max_level=3):
    """index of the deepest level: the pyramid stops before a level of 21 pixels or fewer (buildOpticalFlowPyramid)"""
    lvl = 0
    while lvl < max_level and (w + 1) // 2 > 21 and (h + 1) // 2 > 21:
        w, h, lvl = (w + 1) // 2, (h + 1) // 2, lvl + 1
    return lvl


def refl(n, lo, hi):
    """cv::borderInterpolate(BORDER_REFLECT_101) of indices lo .. hi - 1, repeated for levels narrower than the border"""
    idx = np.arange(lo, hi)
    if n == 1:
        return np.zeros_like(idx)
    period = 2 * (n - 1)
    idx = np.mod(idx, period)
    return np.where(idx >= n, period - idx, idx)


def pack(d):
    """the checker's Scharr image [h, w, 2] as the device stores it: 4 Ix | 4 Iy << 16"""
    d = d.astype(np.int64) * 4
    return ((d[..., 0] & 0xffff) | ((d[..., 1] & 0xffff) << 16)).astype(np.uint32)


def expected_planes(orc, img, max_level=3):
    """[(pix uint8, der uint32)] per level the library builds for this image, whole [rows][stride] planes"""
    h, w = img.shape
    ref = orc.build_pyramid(img, max_level)
    out = []
    for l in range(depth(w, h, max_level) + 1):
        lh, lw = ref[l].shape
        ls = stride(lw)
        pix = np.ascontiguousarray(ref[l][refl(lh, -BY, lh + BY)][:, refl(lw, -BX, ls - BX)])
        der = np.zeros((lh + 2 * BY, ls), np.uint32)
        der[BY:BY + lh, BX:BX + lw] = pack(orc.scharr(ref[l]))
        pix.setflags(write=False)
        der.setflags(write=False)
        out.append((pix, der))
    return out


def noise(shape, seed):
    """uniform noise, (h, w) uint8; images of one batch take consecutive seeds"""
    w, h = shape
    return np.random.default_rng([w, h, seed]).integers(0, 256, (h, w), dtype=np.uint8)


def checker(shape, cell=5):
    """0 / 255 squares of 5 x 5 pixels (a one-pixel checkerboard has no Scharr response at all: x - 1 and x + 1 are equal)"""
    w, h = shape
    yy, xx = np.mgrid[0:h, 0:w]
    return (((xx // cell + yy // cell) % 2) * 255).astype(np.uint8)


def image(shape, k):
    """image k of the shape's set: k = 3 is the checkerboard, every other k noise of its own seed"""
    key = ("image", shape, k)
    if key not in _CACHE:
        _CACHE[key] = checker(shape) if k == 3 else noise(shape, k)
        _CACHE[key].setflags(write=False)
    return _CACHE[key]


def expected(orc, shape, k, max_level=3):
    """expected_planes of image(shape, k), computed once per session and read-only"""
    key = ("planes", shape, k, max_level)
    if key not in _CACHE:
        _CACHE[key] = expected_planes(orc, image(shape, k), max_level)
    return _CACHE[key]


def level_shape(shape, l):
    w, h = shape
    for _ in range(l):
        w, h = (w + 1) // 2, (h + 1) // 2
    return w, h


def premises(shape, planes, is_checker=False):
    """asserted on the expectation alone: the border is not a replicated edge, at the narrow / low levels it is not a single
    reflection either, and der holds positive and negative halves (the checkerboard: the extreme values of both signs)"""
    assert len(planes) == depth(*shape) + 1
    for l, (pix, der) in enumerate(planes):
        lw, lh = level_shape(shape, l)
        assert pix.shape == der.shape == (lh + 2 * BY, stride(lw)) and pix.shape[1] - BX - lw >= BY
        ix, iy = der.view(np.int16)[..., 0::2], der.view(np.int16)[..., 1::2]
        if is_checker:
            if l == 0:  # a full-contrast edge over three rows / columns: 4 * (3 + 10 + 3) * 255, the largest value the plane can hold
                assert ix.max() == iy.max() == 16320 and ix.min() == iy.min() == -16320
            continue
        assert (ix > 0).any() and (ix < 0).any() and (iy > 0).any() and (iy < 0).any(), l
        inner = pix[BY:BY + lh, BX:BX + lw]
        rows, cols = np.clip(np.arange(-BY, lh + BY), 0, lh - 1), np.clip(np.arange(-BX, pix.shape[1] - BX), 0, lw - 1)
        assert not np.array_equal(pix, inner[rows][:, cols]), (l, "replicated edge")

        def once(n, lo, hi):                  # a single reflection, clamped where it leaves the level
            i = np.arange(lo, hi)
            return np.clip(np.where(i < 0, -i, np.where(i >= n, 2 * (n - 1) - i, i)), 0, n - 1)
        single = inner[once(lh, -BY, lh + BY)][:, once(lw, -BX, pix.shape[1] - BX)]
        narrow = lw - 1 < max(BX, pix.shape[1] - BX - lw) or lh - 1 < BY
        assert np.array_equal(pix, single) != narrow, (l, "single reflection", narrow)


def assert_planes(got, want, what):
    """np.array_equal over the whole plane, pix and der, of every level; on a mismatch: where"""
    assert len(got) == len(want), (what, "levels", len(got), len(want))
    for l, ((gp, gd), (wp, wd)) in enumerate(zip(got, want)):
        for name, g, w in (("pix", gp, wp), ("der", gd, wd)):
            assert g.shape == w.shape and g.dtype == w.dtype, (what, l, name, g.shape, w.shape)
            if not np.array_equal(g, w):
                bad = np.argwhere(g != w)
                raise AssertionError((what, "level %d" % l, name, "%d wrong of %d" % (len(bad), g.size), "first (row, column - BX)",
                                      [(int(r) - BY, int(c) - BX) for r, c in bad[:6]], "plane of %d x %d" % (w.shape[1], w.shape[0])))


# ---- the planes of the CPU emulator (tests/host_check/kernel_emu.cpp) ----------------------------------------------------------
REGIMES = {"wide-xcd-order": 2, "thin-dispatch-order": 3}


def emu_lib():
    import emu_build
    from conftest import BUILD_DIR, SAN_FLAGS
    return emu_build.shared("kernel_emu", SAN_FLAGS, BUILD_DIR)


def emu_planes(lib, img, max_level=3, regime=2):
    """the emulated fused passes' planes of one image, each level's heap block as it stands after the build"""
    from conftest import vp
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    out = []
    lib.ke_set_pyr_lds(regime)
    try:
        for l in range(max_level + 1):
            cap = (h + 2 * BY) * stride(w)
            pix, der = np.zeros(cap, np.uint8), np.zeros(cap, np.uint32)
            lw, lh, ls = C.c_int(0), C.c_int(0), C.c_int(0)
            levels = lib.ke_bordered_level(vp(img), w, h, max_level, l, vp(pix), vp(der), cap, C.byref(lw), C.byref(lh), C.byref(ls))
            if levels <= l:
                break
            n = ls.value * (lh.value + 2 * BY)
            out.append((pix[:n].reshape(-1, ls.value), der[:n].reshape(-1, ls.value)))
    finally:
        lib.ke_set_pyr_lds(2)
    return out
