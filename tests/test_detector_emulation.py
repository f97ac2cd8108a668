"""The frame loop's detection under VODET_SHI_TOMASI (include/vo_detector.h) on the CPU: the product's seq_prepare_kernel, the frames
form of corners.hip's three passes and bucket_kernel's split form through the coroutine emulator (tests/host_check/detector_emu.cpp),
in both orders the product launches them (inline, and the look-ahead of the lock-step loop), against appendNewFeatures with
goodFeaturesToTrack from the references and the oracle's bucketingFeatures.  Identity throughout.  The same cases run once as a
stand-alone program under ASan + UBSan."""
import numpy as np
import pytest

import detector_cases as dc


def crops(which, frames=(0,)):
    _, lefts, _ = dc.world_frames()
    return [np.ascontiguousarray(lefts[k][which]) for k in frames]


def case_two_images():
    imgs = crops(dc.CROP_BIG, (0, 1))
    return imgs, [(1,) + dc.EMPTY, (0,) + dc.EMPTY], {}


def case_detect_flag():
    """the middle frame carries as many points as redetect_below: it does not detect again"""
    imgs = crops(dc.CROP_BIG, (0, 1))
    few = dc.carried_set(64, 48, 10, 0, seed=5)
    full = dc.carried_set(64, 48, 30, 3, seed=6)
    return imgs, [(0,) + dc.EMPTY, (1,) + full, (1,) + few], dict(redetect_below=30)


def case_carried_ages(fpb):
    imgs = crops(dc.CROP_BIG)
    return imgs, [(0,) + dc.carried_set(64, 48, 40, 5)], dict(fpb=fpb)


def case_harris5():
    imgs = crops(dc.CROP_BIG)
    return imgs, [(0,) + dc.carried_set(64, 48, 12, 2, seed=8)], dict(det=dc.HARRIS5, fpb=2)


def case_small_crop():
    imgs = crops(dc.CROP_SMALL)
    return imgs, [(0,) + dc.EMPTY], dict(stride=37, bucket_threads=256)


CASES = {"two_images": case_two_images, "detect_flag": case_detect_flag, "carried_ages_fpb1": lambda: case_carried_ages(1),
         "carried_ages_fpb4": lambda: case_carried_ages(4), "harris5": case_harris5, "small_crop": case_small_crop}


def check(got, imgs, frames, kw, lookahead):
    det = kw.get("det", dc.DEFAULT)
    rb = kw.get("redetect_below", 2000)
    for f, (image, pts, ages) in enumerate(frames):
        want_p, want_a, n_new = dc.expected_bucketed(imgs[image], pts, ages, det, rb, kw.get("bucket_size", 0), kw.get("fpb", 1))
        g = got[f]
        assert g["overflow"] == 0 and g["n_new"] == n_new and g["n"] == len(want_p), (f, g["n"], g["n_new"], n_new)
        assert np.array_equal(g["pts"], want_p) and np.array_equal(g["ages"], want_a), f
        assert g["detect"] == (1 if len(pts) < rb else 0)
        if not g["detect"] and not lookahead:   # a frame that does not detect again costs no map, candidate or select pass
            assert g["touched"] == 0 and g["n_cand"] == 0


@pytest.mark.parametrize("lookahead", [False, True], ids=["inline", "lookahead"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_frames_form_and_bucketing(name, lookahead):
    imgs, frames, kw = CASES[name]()
    check(dc.emu_run(imgs, frames, lookahead=lookahead, **kw), imgs, frames, kw, lookahead)


def test_crop_premises():
    """the two crops yield the corner counts the issue states, so that the cases above are about real lists"""
    big, small = crops(dc.CROP_BIG)[0], crops(dc.CROP_SMALL)[0]
    assert big.shape == (48, 64) and small.shape == (32, 32)
    assert len(dc.ref_corners(big)) == 58 and len(dc.ref_corners(small)) == 19


@pytest.mark.parametrize("lookahead", [False, True], ids=["inline", "lookahead"])
def test_candidate_overflow_reaches_the_overflow_flag(lookahead):
    """a candidate list beyond the capacity: the select pass reports lcap + 1 corners, which bucket_kernel's split form turns into bit
    0 of the frame's overflow flag; the frame beside it, whose candidates fit, is complete"""
    flat = np.full((48, 64), 90, np.uint8)
    flat[20:24, 30:34] = 200                       # four corners of one square: a handful of candidates
    imgs = [crops(dc.CROP_BIG)[0], flat]
    frames = [(0,) + dc.EMPTY, (1,) + dc.EMPTY]
    lcap = 32
    assert dc.emu_run(imgs, frames[:1])[0]["n_cand"] > lcap
    got = dc.emu_run(imgs, frames, lcap=lcap, out_cap=512, lookahead=lookahead)
    assert got[0]["n_cand"] > lcap and got[0]["n_new"] == lcap + 1 and got[0]["overflow"] & 1
    want_p, want_a, n_new = dc.expected_bucketed(flat, *dc.EMPTY)
    assert 0 < n_new <= lcap and got[1]["overflow"] == 0 and got[1]["n_new"] == n_new
    assert np.array_equal(got[1]["pts"], want_p) and np.array_equal(got[1]["ages"], want_a)


def test_standalone_under_sanitizers(tmp_path):
    """every case once more, and the overflow case, in the ASan + UBSan program: exit status 0, no report, the same bytes"""
    for name in sorted(CASES):
        imgs, frames, kw = CASES[name]()
        for lookahead in (False, True):
            d = tmp_path / ("%s_%d" % (name, lookahead))
            d.mkdir()
            got = dc.run_standalone(d, imgs, frames, lookahead=lookahead, **kw)
            check(got, imgs, frames, kw, lookahead)
    d = tmp_path / "overflow"
    d.mkdir()
    imgs = crops(dc.CROP_BIG)
    got = dc.run_standalone(d, imgs, [(0,) + dc.EMPTY], lcap=32, out_cap=512)
    assert got[0]["n_new"] == 33 and got[0]["overflow"] & 1
