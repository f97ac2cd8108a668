"""The premises of the frame loop with the Shi-Tomasi detector (include/vo_detector.h), from the references alone -- no product code
runs here: the reference's frame loop with appendNewFeatures' one detector call swapped for goodFeaturesToTrack is healthy on the
suite's small_world, its bucketed sets differ from the FAST loop's in every frame (so a loop that ignored the setting cannot pass the
device tests by accident), and the two crops the device and emulator tests use yield the lists they are chosen for."""
import functools

import numpy as np
import pytest

import detector_cases as dc


@functools.lru_cache(maxsize=None)
def reference_loop(detector, fpb):
    """main.cpp:123-224 over the oracle for the first four frames: per frame (bucketed points, corners found, circular-matching
    survivors, consistency-filter survivors, solvePnPRansac's status, inliers, translation)"""
    from oracle import oracle as orc
    orc.build()
    world, L, R = dc.world_frames()
    P_l, P_r = world.proj_matrices()
    h, w = L[0].shape
    pts, ages = dc.EMPTY
    out = []
    for k in range(4):
        l0, r0, l1, r1 = L[k], R[k], L[k + 1], R[k + 1]
        if detector == "shi_tomasi":
            bp, ba, n_new = dc.expected_bucketed(l0, pts, ages, features_per_bucket=fpb)
        else:
            fast = orc.fast_detect(l0, 20, True)
            n_new = len(fast)
            bp, ba = orc.bucketing_features(h, w, np.vstack([pts, fast]), np.concatenate([ages, np.zeros(n_new, np.int32)]), h // 10, fpb)
        ref = orc.circular_matching(l0, r0, l1, r1, bp, ages=ba)
        (a, b, c, _), _ = orc.check_valid_and_remove(ref["l0"], ref["r0"], ref["l1"], ref["r1"], ref["l0_ret"])
        xyz = orc.triangulate(P_l, P_r, a, b)
        rc, _, tv, inl, _ = orc.solve_pnp_ransac(xyz, c, world.K())
        out.append(dict(bucketed=bp, n_new=n_new, n_circ=ref["n_out"], n_filtered=len(a), rc=rc, n_inliers=len(inl), tvec=tv))
        pts, ages = c, ref["ages"]      # currentVOFeatures: pointsLeft_t1, and the ages deleteUnmatchFeaturesCircle left
    return out


@pytest.mark.parametrize("fpb", [1, 4])
def test_the_shi_tomasi_loop_reaches_the_pose_solve(fpb):
    frames = reference_loop("shi_tomasi", fpb)
    for k, f in enumerate(frames):
        assert 1016 <= f["n_new"] <= 1148, (k, f["n_new"])
        assert f["rc"] == 1 and f["n_inliers"] >= 100, (k, f["rc"], f["n_inliers"])
        if fpb == 1:
            assert 283 <= len(f["bucketed"]) <= 292 and 186 <= f["n_filtered"] <= 197 and 123 <= f["n_inliers"] <= 147, (k, len(f["bucketed"]), f["n_filtered"], f["n_inliers"])
        else:
            assert 914 <= len(f["bucketed"]) <= 1095 and 493 <= f["n_inliers"] <= 583, (k, len(f["bucketed"]), f["n_inliers"])


@pytest.mark.parametrize("fpb", [1, 4])
def test_the_detector_decides_the_bucketed_sets(fpb):
    shi, fast = reference_loop("shi_tomasi", fpb), reference_loop("fast", fpb)
    for k in range(4):
        assert fast[k]["rc"] == 1 and fast[k]["n_new"] > shi[k]["n_new"]
        a, b = shi[k]["bucketed"], fast[k]["bucketed"]
        assert a.shape != b.shape or not np.array_equal(a, b), k
        assert np.abs(shi[k]["tvec"] - fast[k]["tvec"]).max() < 0.05, (k, shi[k]["tvec"], fast[k]["tvec"])   # the same motion all the same


def test_the_crops_of_the_device_and_emulator_tests():
    _, L, _ = dc.world_frames()
    big, small = np.ascontiguousarray(L[0][dc.CROP_BIG]), np.ascontiguousarray(L[0][dc.CROP_SMALL])
    assert big.shape == (48, 64) and small.shape == (32, 32)
    assert len(dc.ref_corners(big)) == 58 and len(dc.ref_corners(small)) == 19
    # the other parameter sets of the tests give other lists on the full image and on the crop
    for img in (L[0], big):
        default = dc.ref_corners(img)
        for det in (dc.FEW, dc.HARRIS5):
            other = dc.ref_corners(img, **det)
            assert len(other) > 0 and (other.shape != default.shape or not np.array_equal(other, default))
    assert len(dc.ref_corners(L[0], **dc.FEW)) == 50
