"""Every byte of the bordered pixel planes and packed Scharr planes pyr_pass_kernel writes on the MI355X, read back whole through
vo_batch_get_level_planes and compared with tests/pyramid_planes.py (which test_pyramid_planes.py holds the CPU emulator to):
the REFLECT_101 border to the end of each row, the zero border of the derivatives, and -- the product lays levels and images back
to back in one allocation -- nothing stored into a neighbouring level or image.  Batch route over the image counts either side of
the thin / wide border items and of the XCD-aware workgroup order, partial rebuilds, reconfiguration of one context, and the
synchronous calls with their two-image route.  Every comparison is np.array_equal on the whole [rows][stride] plane."""
import numpy as np
import pytest

import pyramid_planes as pp

pytestmark = pytest.mark.gpu
MAX_W, MAX_H = max(s[0] for s in pp.SHAPES), max(s[1] for s in pp.SHAPES)


@pytest.fixture(scope="module")
def ctx(volib):
    c = volib.Context(0, MAX_W, MAX_H, 64, 4)       # 6 images per frame: 24
    yield c
    c.close()


def read_planes(ctx, idx, n_levels):
    return [ctx.batch_get_level_planes(idx, l) for l in range(n_levels)]


def build(ctx, volib, shape, seeds, first=None, count=None):
    """upload image(shape, seeds[i]) into slot i for every i given, rebuild the range (default: every image), wait"""
    for i, k in seeds.items():
        ctx.batch_upload_image(i, pp.image(shape, k))
    if first is not None:
        ctx.batch_set_pyramid_range(first, count)
    ctx.batch_run(volib.STAGE_PYRAMID)
    ctx.batch_sync()


CASES = [(s, n) for s in pp.SHAPES for n in (pp.COUNTS if s in pp.BIG else (4, 17))]


@pytest.mark.parametrize("shape,n_images", CASES, ids=["%s-%d" % (pp.ids(s), n) for s, n in CASES])
def test_batch_route(ctx, volib, orc, shape, n_images):
    w, h = shape
    n_levels = pp.depth(w, h) + 1
    ctx.batch_configure(n_images, w, h, 4)
    build(ctx, volib, shape, {i: i for i in range(n_images)})
    for i in range(n_images):
        pp.assert_planes(read_planes(ctx, i, n_levels), pp.expected(orc, shape, i), (shape, n_images, "image %d" % i))
    with pytest.raises(volib.VoError):
        ctx.batch_get_level_planes(0, n_levels)
    with pytest.raises(volib.VoError):
        ctx.batch_get_level_planes(n_images, 0)


def test_range_rebuild(ctx, volib, orc):
    """vo_batch_set_pyramid_range: 8 images (a thin launch in dispatch order), then 16 (a wide one in XCD-aware order), of 24; the
    images of the range hold the new pictures' planes, every plane of every other image is what it was"""
    shape, n = (131, 97), 24
    n_levels = pp.depth(*shape) + 1
    ctx.batch_configure(n, *shape, 4)
    seeds = {i: i for i in range(n)}
    build(ctx, volib, shape, seeds)
    before = [read_planes(ctx, i, n_levels) for i in range(n)]
    for i in range(n):
        pp.assert_planes(before[i], pp.expected(orc, shape, i), ("all 24", i))
    for first, count, base in ((5, 8, 100), (4, 16, 200)):
        new = {i: base + i for i in range(first, first + count)}
        build(ctx, volib, shape, new, first, count)
        seeds.update(new)
        for i in range(n):
            got = read_planes(ctx, i, n_levels)
            if i in new:
                pp.assert_planes(got, pp.expected(orc, shape, seeds[i]), ("range %d + %d" % (first, count), i))
                assert not np.array_equal(got[0][0], before[i][0][0])
            else:
                pp.assert_planes(got, before[i], ("outside range %d + %d" % (first, count), i))
            before[i] = got


def test_reconfigure(volib, orc):
    """one context through 169 x 169, 47 x 45, 169 x 169 with other pictures, two levels and four again: the planes are right
    after every step -- der zero outside the image where a plane of the previous layout held derivatives"""
    c = volib.Context(0, 169, 169, 64, 1)
    try:
        steps = (((169, 169), 3, 0), ((47, 45), 3, 10), ((169, 169), 3, 20), ((169, 169), 1, 30), ((169, 169), 3, 40))
        for shape, max_level, base in steps:
            if max_level != c.get_params().lk_max_level:
                c.set_params(lk_max_level=max_level)
            c.batch_configure(4, *shape, 1)
            build(c, volib, shape, {i: base + i for i in range(4)})
            n_levels = min(pp.depth(*shape), max_level) + 1
            for i in range(4):
                want = pp.expected(orc, shape, base + i, max_level)
                assert len(want) == n_levels
                pp.assert_planes(read_planes(c, i, n_levels), want, (shape, max_level, i))
            with pytest.raises(volib.VoError):
                c.batch_get_level_planes(0, n_levels)
    finally:
        c.close()


def test_synchronous_calls(volib, orc):
    """vo_circular_match with four images, then twice on the kept pair (two images, built on the filter stream beside hop 0):
    the new pair's two slots hold its planes, the other two are byte for byte what they were"""
    shape = (131, 97)
    n_levels = pp.depth(*shape) + 1
    pts = np.array([[10, 10], [0, 0], [130, 96], [65.5, 48.25], [129.5, 3], [2, 95.5]], np.float32)
    c = volib.Context(0, *shape, 64, 1)
    try:
        c.circular_match(*(pp.image(shape, k) for k in range(4)), pts)
        slots = [read_planes(c, i, n_levels) for i in range(4)]
        for i in range(4):
            pp.assert_planes(slots[i], pp.expected(orc, shape, i), ("four images", i))
        new, kept = (0, 1), (2, 3)            # (the first call left its t1 pair in slots 2, 3; the next pair goes to t0 ^ 2)
        for call, base in ((1, 50), (2, 60)):
            c.circular_match(None, None, pp.image(shape, base), pp.image(shape, base + 1), pts)
            for j, i in enumerate(new):
                got = read_planes(c, i, n_levels)
                pp.assert_planes(got, pp.expected(orc, shape, base + j), ("kept-pair call %d" % call, i))
                slots[i] = got
            for i in kept:
                pp.assert_planes(read_planes(c, i, n_levels), slots[i], ("kept-pair call %d, kept slot" % call, i))
            new, kept = kept, new
    finally:
        c.close()
