"""The premises of the frame loop's top-up under a mask of the carried points (include/vo_topup.h), from the references alone -- no
product code runs here.  They are asserted so that a loop which ignored the setting, or read the mask the wrong way ("detect unmasked,
filter afterwards", or a threshold from the unmasked maximum), cannot pass the emulator and device tests by accident: on the suite's
small_world the three readings give three different lists, the all-zero mask gives none, and the reference loop with the masked call
is healthy and differs from the unmasked loop from frame 1 on."""
import functools

import numpy as np
import pytest

import corners_mask_cases as cm
import detector_cases as dc
import test_detector_ref as tdr
import topup_cases as tc


def counts(img, carried, radius, det=tc.DEFAULT):
    return len(tc.ref_topup_corners(img, carried, radius, det)), len(dc.ref_corners(img, **det)), len(tc.filtered_afterwards(img, carried, radius, det))


def test_the_masked_maximum_lowers_the_threshold():
    """the strongest corners carried: the maximum over the allowed pixels is smaller, so MORE corners pass than without a mask"""
    img = tc.L0()
    assert counts(img, tc.strongest(img, 1), 5) == (1054, 1016, 1015)
    assert counts(img, tc.strongest(img, 8), 5) == (1214, 1016, 1003)


def test_a_random_carried_set():
    img = tc.L0()
    assert counts(img, tc.carried_set(480, 160, 40, 5)[0], 5) == (977, 1016, 970)


def test_the_all_zero_mask():
    small = tc.crop(tc.CROP_SMALL)
    kept = tc.carried_set(32, 32, 40, 5)[0]
    assert small.shape == (32, 32) and not cm.ref_disc_mask(32, 32, kept, 10).any()
    assert len(tc.ref_topup_corners(small, kept, 10)) == 0


def test_harris5():
    img = tc.L0()
    got = counts(img, tc.strongest(img, 1, tc.HARRIS5), 5, tc.HARRIS5)
    assert got[:2] == (384, 322)


def test_the_crops():
    assert tc.crop(tc.CROP_BIG).shape == (48, 64) and tc.crop(tc.CROP_ODD).shape == (47, 61) and (61 * 47) % 2 == 1
    for which in (tc.CROP_BIG, tc.CROP_ODD):   # the mask decides on the crops too
        img = tc.crop(which)
        h, w = img.shape
        kept = tc.carried_set(w, h, 10, 2, seed=5)[0]
        a, b = tc.ref_topup_corners(img, kept, 5), dc.ref_corners(img)
        assert len(a) > 0 and (a.shape != b.shape or not np.array_equal(a, b))


@functools.lru_cache(maxsize=None)
def reference_loop(fpb, radius):
    """test_detector_ref.reference_loop with the detector call under the disc mask of the carried points"""
    from oracle import oracle as orc
    orc.build()
    world, L, R = dc.world_frames()
    P_l, P_r = world.proj_matrices()
    pts, ages = dc.EMPTY
    out = []
    for k in range(4):
        l0, r0, l1, r1 = L[k], R[k], L[k + 1], R[k + 1]
        bp, ba, n_new = tc.expected_bucketed(l0, pts, ages, radius, features_per_bucket=fpb)
        ref = orc.circular_matching(l0, r0, l1, r1, bp, ages=ba)
        (a, b, c, _), _ = orc.check_valid_and_remove(ref["l0"], ref["r0"], ref["l1"], ref["r1"], ref["l0_ret"])
        xyz = orc.triangulate(P_l, P_r, a, b)
        rc, _, tv, inl, _ = orc.solve_pnp_ransac(xyz, c, world.K())
        out.append(dict(bucketed=bp, n_new=n_new, rc=rc, n_inliers=len(inl), tvec=tv))
        pts, ages = c, ref["ages"]
    return out


def test_the_reference_loop_with_the_top_up():
    top, plain = reference_loop(1, 5), tdr.reference_loop("shi_tomasi", 1)
    assert [f["n_new"] for f in top] == [1016, 935, 900, 900]
    assert [len(f["bucketed"]) for f in top] == [283, 287, 287, 291]
    assert [(f["rc"], f["n_inliers"]) for f in top] == [(1, 141), (1, 147), (1, 128), (1, 133)]
    assert np.array_equal(top[0]["bucketed"], plain[0]["bucketed"])     # nothing is carried into frame 0
    for k in range(1, 4):
        a, b = top[k]["bucketed"], plain[k]["bucketed"]
        assert a.shape != b.shape or not np.array_equal(a, b), k
    for k in range(4):
        assert np.abs(top[k]["tvec"] - plain[k]["tvec"]).max() < 0.05, (k, top[k]["tvec"], plain[k]["tvec"])


def test_the_reference_loop_at_four_per_bucket_and_radius_10():
    top = reference_loop(4, 10)
    assert [f["n_new"] for f in top] == [1016, 82, 169, 172]
    assert all(f["rc"] == 1 for f in top)
