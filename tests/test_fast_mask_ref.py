"""The premises of cv::FAST under a mask (include/vo_fast_mask.h), on the references alone: oracle.fast_detect, runByPixelsMask restated in
numpy, ref_disc_mask and the oracle's bucketingFeatures (fast_mask_cases.py).  On the suite's 480 x 160 L[0] the mask of the carried
points decides something -- corners leave, and the bucketed set changes --, non-maximum suppression runs on the unmasked image, an
all-zero mask leaves nothing, and the empty carried set is the unmasked composition.  No product code runs here."""
import numpy as np

import corners_mask_cases as cm
import fast_mask_cases as fm

# what the oracle gives on L[0] with corners[::40] (41 points) carried, at radius 5 and 10
REMOVED_R5, REMOVED_R10 = 118, 338


def test_the_mask_of_the_carried_points_removes_corners_on_L0():
    img = fm.L0()
    h, w = img.shape
    assert (w, h) == (480, 160)
    corners = fm.ref_fast(img)
    assert len(corners) == 1603
    carried, _ = fm.every_nth(img, 40)
    assert len(carried) == 41
    m5, m10 = cm.ref_disc_mask(w, h, carried, 5), cm.ref_disc_mask(w, h, carried, 10)
    k5, k10 = fm.ref_masked(img, m5), fm.ref_masked(img, m10)
    assert len(corners) - len(k5) == REMOVED_R5 and len(corners) - len(k10) == REMOVED_R10
    # every carried point is itself a corner, so each is among the removed; the survivors keep FAST's row-major order
    assert not (set(map(tuple, carried)) & set(map(tuple, k5)))
    key = k5[:, 1].astype(np.int64) * w + k5[:, 0].astype(np.int64)
    assert np.all(np.diff(key) > 0)
    assert fm.crop(fm.CROP_SMALL).shape == (32, 32) and len(fm.ref_fast(fm.crop(fm.CROP_SMALL))) == 14
    assert fm.crop(fm.CROP_BIG).shape == (48, 64) and len(fm.ref_fast(fm.crop(fm.CROP_BIG))) == 72


def test_the_bucketed_set_differs_from_the_unmasked_one():
    img = fm.L0()
    carried, ages = fm.every_nth(img, 40)
    for fpb in (1, 4):
        p0, a0, n0 = fm.expected_bucketed(img, carried, ages, None, features_per_bucket=fpb)
        p1, a1, n1 = fm.expected_bucketed(img, carried, ages, 5, features_per_bucket=fpb)
        assert (n0, n1) == (1603, 1603 - REMOVED_R5)
        assert p0.shape != p1.shape or not np.array_equal(p0, p1), fpb


def test_a_masked_suppressor_does_not_resurrect_its_neighbour():
    """non-maximum suppression runs on the unmasked image: masking the pixel of a kept corner (radius 0) removes that corner and
    nothing comes back next to it"""
    img = fm.L0()
    h, w = img.shape
    kept = fm.ref_fast(img)
    every = fm.ref_fast(img, nonmax=False)
    kept_set = set(map(tuple, kept.astype(int)))
    pair = None
    for x, y in every.astype(int):
        if (x, y) in kept_set:
            continue
        near = [(x + dx, y + dy) for dx in (-1, 0, 1) for dy in (-1, 0, 1) if (dx or dy) and (x + dx, y + dy) in kept_set]
        if near:
            pair = ((x, y), near[0])
            break
    assert pair is not None, "L[0] has a corner that its neighbour suppresses"
    (sx, sy), (kx, ky) = pair
    carried = np.array([(kx, ky)], np.float32)
    got = fm.ref_topup_corners(img, carried, 0)
    want = kept[~((kept[:, 0] == kx) & (kept[:, 1] == ky))]
    assert len(want) == len(kept) - 1 and np.array_equal(got, want)
    assert (sx, sy) not in set(map(tuple, got.astype(int)))
    # ... whereas FAST on an image whose suppressor is gone would be another detector: the composition is filter-afterwards
    assert np.array_equal(got, fm.run_by_pixels_mask(kept, cm.ref_disc_mask(w, h, carried, 0)))


def test_an_all_zero_mask_gives_no_corners():
    img = fm.crop(fm.CROP_SMALL)
    assert len(fm.ref_masked(img, np.zeros(img.shape, np.uint8))) == 0
    pts, ages = fm.carried_set(32, 32, 40, 5)
    assert not cm.ref_disc_mask(32, 32, pts, 10).any()
    p, a, n_new = fm.expected_bucketed(img, pts, ages, 10)
    assert n_new == 0
    from oracle import oracle as orc
    p0, a0 = orc.bucketing_features(32, 32, pts, ages, 3, 1)
    assert np.array_equal(p, p0) and np.array_equal(a, a0)


def test_the_empty_carried_set_is_the_unmasked_composition():
    for img in (fm.crop(fm.CROP_BIG), fm.L0()):
        a = fm.expected_bucketed(img, *fm.EMPTY, 5)
        b = fm.expected_bucketed(img, *fm.EMPTY, None)
        assert a[2] == b[2] == len(fm.ref_fast(img))
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    # and an all-255 mask filters nothing
    img = fm.crop(fm.CROP_ODD)
    assert np.array_equal(fm.ref_masked(img, np.full(img.shape, 255, np.uint8)), fm.ref_fast(img))
    assert np.array_equal(fm.ref_masked(img, np.full(img.shape, 1, np.uint8)), fm.ref_fast(img))   # (any non-zero byte allows)
