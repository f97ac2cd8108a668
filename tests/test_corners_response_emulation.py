"""The product's response kernels (visual_odom_amd/csrc/corners.hip: corn_map_resp_kernel<5, 0>, <3, 1>, <5, 1>, then the
candidate and select kernels on whatever map comes in) run on the CPU through the coroutine emulator
(tests/host_check/corners_response_emu.cpp) and held BIT FOR BIT -- maps and corner lists with their order -- to
tests/host_check/corners_response_ref.c.  Every image and every mask sits in a heap block of exactly (h - 1) * stride + w bytes, the
mask stride differs from the image stride, and the last test runs the same harness as a stand-alone ASan + UBSan program.  CPU only."""
import numpy as np
import pytest

import corners_emu as ce
import corners_mask_cases as cm
import corners_response_cases as cr
import corners_response_fuzz_cases as fz

# (3, 3): one column wider than the B = 5 halo, the smallest REFLECT_101 takes two deep; (253, 9) and (504, 6): one column past a
# workgroup's 252 at B = 5 (and one short of 254 at B = 3), and exactly two workgroups' worth
SHAPES = [(3, 3), (5, 5), (6, 7), (17, 13), (65, 17), (131, 67), (253, 9), (504, 6)]


def same(got, want, what):
    assert (got[1], got[2]) == (want[1], want[2]), what
    assert got[0].tobytes() == want[0].tobytes(), "%s: corner list or its order differs" % (what,)


@pytest.mark.parametrize("block,harris", cr.RESPONSES)
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_maps_and_corners_bit_for_bit(shape, block, harris):
    w, h = shape
    for name, img in (("noise", ce.noise(w, h, 31)), ("blobs", ce.blobs(w, h, 32)), ("dark", ce.dark_highlights(w, h, 33)), ("one_sided", cr.one_sided(w, h, 34))):
        want = cr.ref_map(img, block, harris)
        assert np.array_equal(cr.bits(cr.emu_map(img, block, harris, stride=w + 3)), cr.bits(want)), name
        for md, mc in ((0.0, 0), (5.0, 0), (1.5, 7)):
            got = cr.emu_detect([img], None, mc, 0.01, md, block, harris, stride=w + 5)[0]
            same(got, cr.ref_detect(img, None, mc, 0.01, md, block, harris), (name, md, mc))
            assert np.array_equal(cr.bits(got[3]), cr.bits(want)), name


def test_default_response_is_the_existing_kernels():
    w, h = 65, 17
    img, mask = ce.noise(w, h, 3), cm.checker(w, h)
    assert np.array_equal(cr.bits(cr.emu_map(img, 3, 0)), cr.bits(ce.emu_map(img)))
    same(cr.emu_detect([img], None, 0, 0.01, 5.0, 3, 0)[0], ce.emu_detect([img], 0, 0.01, 5.0)[0], "no mask")
    same(cr.emu_detect([img], [mask], 0, 0.01, 5.0, 3, 0)[0], cm.emu_detect([img], [mask], 0, 0.01, 5.0)[0], "mask")


@pytest.mark.parametrize("block,harris", cr.RESPONSES)
def test_masks_and_a_batch_whose_range_starts_at_one(block, harris):
    w, h = 65, 33
    for name, img, mask, mc, q, md in cm.mask_cases(w, h):
        same(cr.emu_detect([img], [mask], mc, q, md, block, harris, stride=w + 3, mask_stride=w + 6)[0],
             cr.ref_detect(img, mask, mc, q, md, block, harris), name)
    imgs = [ce.noise(w, h, 7), ce.blobs(w, h, 8), ce.squares(w, h, 9)]
    masks = [cm.checker(w, h), None, cm.left_half(w, h)]
    for s, got in enumerate(cr.emu_detect(imgs, masks, 0, 0.01, 5.0, block, harris, first=1, n=2, stride=w + 7, mask_stride=w + 9)):
        same(got, cr.ref_detect(imgs[1 + s], masks[1 + s], 0, 0.01, 5.0, block, harris), 1 + s)


def test_adversarial_contents():
    for block in (3, 5):
        ramp = cr.ramp(32, 32)                                    # the negative maximum
        assert cr.emu_detect([ramp], None, 0, 0.01, 0.0, block, 1)[0][1:3] == (0, 0)
        got = cr.emu_detect([ramp], None, 0, 3.0, 0.0, block, 1)[0]
        same(got, cr.ref_detect(ramp, None, 0, 3.0, 0.0, block, 1), "ramp")
        assert got[1] == 840
        same(cr.emu_detect([ramp], None, 0, 3.0, 5.0, block, 1)[0], cr.ref_detect(ramp, None, 0, 3.0, 5.0, block, 1), "ramp, thinned")
        same(cr.emu_detect([ramp], [cm.left_half(32, 32)], 0, 3.0, 2.0, block, 1)[0], cr.ref_detect(ramp, cm.left_half(32, 32), 0, 3.0, 2.0, block, 1), "ramp, mask")
        img = ce.noise(65, 17, 5)
        for k in cr.HARRIS_KS:
            assert np.array_equal(cr.bits(cr.emu_map(img, block, 1, k)), cr.bits(cr.ref_map(img, block, 1, k))), k
            same(cr.emu_detect([img], None, 0, 0.01, 5.0, block, 1, k)[0], cr.ref_detect(img, None, 0, 0.01, 5.0, block, 1, k), k)


def test_a_few_fuzz_cases_and_the_capacity_of_all():
    cases = fz.cases()
    assert len(cases) == fz.N_CASES and {(c["block"], c["harris"]) for c in cases} == set(fz.RESPONSES)
    masked = 0
    for i, c in enumerate(cases):
        img = np.ascontiguousarray(c["img"])
        ncand = cr.ref_detect(img, c["mask"], 1, c["q"], 0.0, c["block"], c["harris"], c["k"])[2]
        assert ncand <= 16384, "every case fits the smallest corner-list capacity of a context"
        masked += c["mask"] is not None
        if i % 10 == 3:
            wmap, wpts, n = fz.expected(c)
            got = cr.emu_detect([img], None if c["mask"] is None else [c["mask"]], c["mc"], c["q"], c["md"], c["block"], c["harris"], c["k"],
                                stride=c["img"].strides[0] + 1, mask_stride=img.shape[1] + 9)[0]
            assert got[1] == n and got[0].tobytes() == wpts.tobytes() and np.array_equal(cr.bits(got[3]), cr.bits(wmap)), i
    assert 15 <= masked <= 50


def test_standalone_under_asan_and_ubsan(tmp_path):
    """the same harness as a stand-alone program built with -fsanitize=address,undefined, run as a child: images, masks, maps and
    lists in exactly sized heap blocks, a list that is exactly full, two map workgroups at B = 5 with a partial second one"""
    w, h = 253, 9
    imgs = [ce.noise(w, h, 9), ce.periodic(w, h), ce.blobs(w, h, 4)]
    masks = [cm.random_half(w, h), None, cm.checker(w, h)]
    for block, harris in cr.RESPONSES:
        lcap = max(cr.ref_detect(i, m, 0, 0.01, 6.0, block, harris)[2] for i, m in zip(imgs, masks))
        one, res = cr.run_standalone(tmp_path, imgs, masks, 0, 0.01, 6.0, block, harris, cr.K, cap=lcap, lcap=lcap, stride=w + 3, mask_stride=w + 5)
        assert np.array_equal(cr.bits(one), cr.bits(cr.ref_map(imgs[0], block, harris)))
        for img, mask, got in zip(imgs, masks, res):
            same(got, cr.ref_detect(img, mask, 0, 0.01, 6.0, block, harris), "stand-alone")
            assert np.array_equal(cr.bits(got[3]), cr.bits(cr.ref_map(img, block, harris)))
    small = [ce.noise(5, 5, 2)]
    one, res = cr.run_standalone(tmp_path, small, None, 0, 0.01, 0.0, 5, 1, cr.K, cap=25, lcap=25, stride=5, mask_stride=5)
    assert np.array_equal(cr.bits(one), cr.bits(cr.ref_map(small[0], 5, 1)))
    same(res[0], cr.ref_detect(small[0], None, 0, 0.01, 0.0, 5, 1), "5 x 5")
