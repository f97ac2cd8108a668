"""The product's Shi-Tomasi kernels (visual_odom_amd/csrc/corners.hip) run on the CPU through the coroutine emulator
(tests/host_check/corners_emu.cpp) and held BIT FOR BIT to the restatement of OpenCV (tests/host_check/corners_ref.c): the whole
quality map with its border pixels, the candidate count, and the corner list with its order.  Shapes from 3 x 3 to three tiles by
five, a row stride that is not the width, a batch of different images, and the contents the detector can get wrong.  The last test
runs the same harness as a stand-alone ASan + UBSan program.  CPU only."""
import numpy as np
import pytest

import corners_emu as ce

CONTENTS = [("noise", lambda w, h: ce.noise(w, h, 1)), ("blobs", lambda w, h: ce.blobs(w, h, 2)), ("squares", lambda w, h: ce.squares(w, h, 3)),
            ("periodic", lambda w, h: ce.periodic(w, h)), ("dark_highlights", lambda w, h: ce.dark_highlights(w, h, 5))]
DISTANCES = [0.0, 1.0, 5.0, 10.5, 32.0]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_as_ref(img, got, max_corners, q, md, cap=None):
    pts, n, ncand, _ = got
    rpts, rn, rcand = ce.ref_detect(img, max_corners, q, md, cap=cap)
    assert (n, ncand) == (rn, rcand)
    assert np.array_equal(pts, rpts), "corner list or its order differs"


@pytest.mark.parametrize("shape", ce.SHAPES, ids=["%dx%d" % s for s in ce.SHAPES])
def test_map_and_corners_bit_for_bit(shape):
    w, h = shape
    for name, gen in CONTENTS:
        img = gen(w, h)
        ref = ce.ref_map(img)
        assert np.array_equal(bits(ce.emu_map(img, stride=w + 5)), bits(ref)), name   # border pixels included, stride != width
        assert np.array_equal(bits(ce.emu_map(img)), bits(ref)), name
        for md in DISTANCES:
            same_as_ref(img, ce.emu_detect([img], 0, 0.01, md, stride=w + 3)[0], 0, 0.01, md)


def test_batch_of_different_images_and_a_range_that_starts_at_one():
    w, h = 65, 17
    imgs = [ce.noise(w, h, 7), ce.blobs(w, h, 8), ce.squares(w, h, 9), ce.periodic(w, h)]
    for s, got in enumerate(ce.emu_detect(imgs, 0, 0.01, 5.0, stride=w + 7)):
        same_as_ref(imgs[s], got, 0, 0.01, 5.0)
    for s, got in enumerate(ce.emu_detect(imgs, 0, 0.01, 5.0, first=1, n=2)):
        same_as_ref(imgs[1 + s], got, 0, 0.01, 5.0)


def test_summation_order_of_the_box_filter_is_upstreams():
    """on a dark frame with highlights above a flat area the running column sum of ColumnSum<double, float> and a plain three-term
    sum give different bits (the ref can do both); the kernel gives the running sum's"""
    img = ce.dark_highlights(131, 67, 0)
    running, plain = ce.ref_map(img), ce.ref_map(img, order=1)
    assert int((bits(running) != bits(plain)).sum()) >= 20
    assert (running[50:] != 0).any() and not plain[50:, 3:-3].any()   # the residual in the flat rows
    assert np.array_equal(bits(ce.emu_map(img, stride=140)), bits(running))
    same_as_ref(img, ce.emu_detect([img], 0, 0.01, 5.0)[0], 0, 0.01, 5.0)


def test_map_maximum_on_a_border_pixel():
    img = ce.border_max(65, 17)
    ref = ce.ref_map(img)
    y, x = np.unravel_index(int(np.argmax(ref)), ref.shape)
    assert y == 0, "the case is built so that the maximum -- which sets the threshold and is never a candidate -- is a border pixel"
    inner_max = float(ref[1:-1, 1:-1].max())
    assert np.array_equal(bits(ce.emu_map(img)), bits(ref))
    same_as_ref(img, ce.emu_detect([img], 0, 0.01, 5.0)[0], 0, 0.01, 5.0)
    # a threshold just above the interior's best value: a maximum taken over the interior alone would leave corners, the whole
    # map's leaves none
    q = 1.05 * inner_max / float(ref.max())
    assert q < 1 and ce.ref_detect(img, 0, 0.01, 5.0)[1] > 0
    got = ce.emu_detect([img], 0, q, 5.0)[0]
    same_as_ref(img, got, 0, q, 5.0)
    assert got[1] == 0


def test_one_sided_border_reflects_the_cov_image_not_the_source():
    """the trap of corners_ref.c step 2: computed from the reflected source, dx dy has the wrong sign on a one-sided border, and here
    that changes the corners -- the ref with the trap switched on shows it; the kernel must agree with the ref without it"""
    img = ce.noise(17, 13, 2)
    good, trapped = ce.ref_map(img), ce.ref_map(img, trap=1)
    diff = good != trapped
    assert diff[:, 0].any() and diff[1:-1, 0].any() and not diff[2:-2, 2:-2].any()   # one-sided (left edge, away from the corners) only
    assert not np.array_equal(ce.ref_detect(img, 0, 0.05, 0.0)[0], ce.ref_detect(img, 0, 0.05, 0.0, trap=1)[0]), "the trap changes a corner"
    assert np.array_equal(bits(ce.emu_map(img)), bits(good))
    same_as_ref(img, ce.emu_detect([img], 0, 0.05, 0.0)[0], 0, 0.05, 0.0)


def test_periodic_pattern_with_exact_ties_follows_the_address_rule():
    img = ce.periodic(64, 32)
    got = ce.emu_detect([img], 0, 0.01, 0.0)[0]
    same_as_ref(img, got, 0, 0.01, 0.0)
    ref = ce.ref_map(img)
    vals = [ref[int(y), int(x)] for x, y in got[0]]
    ties = [i for i in range(len(vals) - 1) if vals[i] == vals[i + 1]]
    assert len(ties) >= 8, "the lattice's interior dots tie exactly"
    addr = [int(y) * 64 + int(x) for x, y in got[0]]
    assert all(addr[i] > addr[i + 1] for i in ties)
    same_as_ref(img, ce.emu_detect([img], 0, 0.01, 10.5)[0], 0, 0.01, 10.5)


def test_dependency_chain_takes_many_rounds():
    """44 dots 4 pixels apart, each fainter than the one before, min_distance 6: every dot conflicts with its better neighbour only,
    so the serial loop's accept / reject alternates along the row and each decision waits for the previous one"""
    img = ce.chain(200, 9, 44, 4)
    got = ce.emu_detect([img], 0, 0.01, 6.0)[0]
    same_as_ref(img, got, 0, 0.01, 6.0)
    assert got[2] == 44 and got[1] == 22
    assert got[3] >= 32, "rounds the suppression took"


def test_max_corners_and_cap():
    img = ce.noise(131, 67, 4)
    full = ce.ref_detect(img, 0, 0.01, 5.0)
    assert full[1] > 40
    for mc in (1, 17, full[1], full[1] + 5):
        same_as_ref(img, ce.emu_detect([img], mc, 0.01, 5.0)[0], mc, 0.01, 5.0)
    same_as_ref(img, ce.emu_detect([img], 17, 0.01, 0.0)[0], 17, 0.01, 0.0)
    got = ce.emu_detect([img], 0, 0.01, 5.0, cap=9)[0]
    assert got[1] == full[1] and np.array_equal(got[0], full[0][:9])           # cap < n: n is reported, cap are written


def test_candidate_overflow_is_reported():
    img = ce.noise(65, 17, 9)
    ncand = ce.ref_detect(img, 0, 0.01, 5.0)[2]
    assert ce.emu_detect([img], 0, 0.01, 5.0, lcap=ncand - 1)[0][1] == -1       # one too many: the overflow mark, no corners
    same_as_ref(img, ce.emu_detect([img], 0, 0.01, 5.0, lcap=ncand)[0], 0, 0.01, 5.0)   # exactly full is fine
    both = ce.emu_detect([img, ce.blobs(65, 17, 1)], 0, 0.01, 5.0, lcap=ncand - 1)
    assert both[0][1] == -1
    same_as_ref(ce.blobs(65, 17, 1), both[1], 0, 0.01, 5.0)                     # the other image of the run is untouched by it


def test_standalone_under_asan_and_ubsan(tmp_path):
    """the same harness as a stand-alone program built with -fsanitize=address,undefined, run as a child: every image and every
    list in an exactly sized heap block, a list one candidate short of overflowing, a partial tile in both directions"""
    w, h = 65, 17
    imgs = [ce.noise(w, h, 9), ce.periodic(w, h), ce.chain(w, h, 12, 4)]
    lcap = max(ce.ref_detect(i, 0, 0.01, 6.0)[2] for i in imgs)
    eig, res = ce.run_standalone(tmp_path, imgs, 0, 0.01, 6.0, cap=lcap, lcap=lcap, stride=w + 3)
    assert np.array_equal(bits(eig), bits(ce.ref_map(imgs[0])))
    for img, got in zip(imgs, res):
        same_as_ref(img, got, 0, 0.01, 6.0, cap=lcap)
