"""The frame loop's detection with the top-up under a mask of the carried points (include/vo_topup.h) on the CPU: the product's
seq_prepare_kernel, the map pass with a null max_key, corn_disc_frames_kernel, corn_max_frames_kernel, the candidate pass under the
plane table, the select pass and bucket_kernel's split form through the coroutine emulator (tests/host_check/topup_emu.cpp), in both
orders the product launches them (inline, and the map pass one step early as the lock-step loop's look-ahead), against the
composition of topup_cases.py: the header's disc mask, goodFeaturesToTrack under it from corners_response_ref.c, appendNewFeatures'
list rule and the oracle's bucketingFeatures.  Identity throughout -- the bucketed sets, the planes against ref_disc_mask, and
corn_max_frames_kernel's key against corn_map_body run under the same plane.  The same cases run once as a stand-alone program under
ASan + UBSan."""
import numpy as np
import pytest

import corners_mask_cases as cm
import detector_cases as dc
import topup_cases as tc


def case_two_images():
    imgs = [tc.crop(tc.CROP_BIG, 0), tc.crop(tc.CROP_BIG, 1)]
    return imgs, [(1,) + tc.carried_set(64, 48, 10, 2, seed=5), (0,) + tc.carried_set(64, 48, 14, 0, seed=6)], {}


def case_detect_flag():
    """the middle frame carries as many points as redetect_below: it does not detect again, and nothing of it is touched"""
    imgs = [tc.crop(tc.CROP_BIG, 0), tc.crop(tc.CROP_BIG, 1)]
    few = tc.carried_set(64, 48, 10, 0, seed=5)
    full = tc.carried_set(64, 48, 30, 3, seed=6)
    return imgs, [(0,) + tc.carried_set(64, 48, 7, 1, seed=7), (1,) + full, (1,) + few], dict(redetect_below=30)


def case_empty_carried():
    return [tc.crop(tc.CROP_BIG)], [(0,) + tc.EMPTY], {}


def case_all_zero_mask():
    return [tc.crop(tc.CROP_SMALL)], [(0,) + tc.carried_set(32, 32, 40, 5)], dict(radius=10, stride=37, bucket_threads=256)


def case_skipped_points():
    """NaN, +-inf, |coordinate| >= 2^30 are skipped; centres outside the image clear what of their disc lies inside"""
    w, h = 64, 48
    pts = np.array([(np.nan, 5.0), (5.0, np.inf), (-np.inf, 3.0), (1e20, 4.0), (4.0, -1e20), (2.0 ** 30, 3.0), (-2.0 ** 30, 3.0), (20.5, 11.5), (-3.0, h / 2),
                    (w + 2.0, h / 2), (w / 2, -4.0), (w / 2, h + 5.0), (-100.0, 5.0), (40.2, 30.7)], np.float32)
    return [tc.crop(tc.CROP_BIG)], [(0, pts, np.arange(len(pts) + 2, dtype=np.int32) % 13)], dict(radius=7)


def case_radius(r):
    return [tc.crop(tc.CROP_BIG)], [(0,) + tc.carried_set(64, 48, 12, 2, seed=8)], dict(radius=r)


def case_harris5():
    return [tc.crop(tc.CROP_BIG)], [(0,) + tc.carried_set(64, 48, 12, 2, seed=8)], dict(det=tc.HARRIS5, fpb=2)


def case_odd_crop():
    """61 x 47: the second frame's map starts 12 bytes behind a 16-byte boundary, and both runs have a head and a tail"""
    imgs = [tc.crop(tc.CROP_ODD, 0), tc.crop(tc.CROP_ODD, 1)]
    return imgs, [(0,) + tc.carried_set(61, 47, 9, 1, seed=4), (1,) + tc.carried_set(61, 47, 11, 0, seed=9)], dict(fpb=4)


def case_full_image():
    """480 x 160: corn_max_frames_kernel over several workgroups"""
    return [tc.L0()], [(0,) + tc.carried_set(480, 160, 40, 5)], {}


CASES = {"two_images": case_two_images, "detect_flag": case_detect_flag, "empty_carried": case_empty_carried, "all_zero_mask": case_all_zero_mask,
         "skipped_points": case_skipped_points, "radius_0": lambda: case_radius(0), "radius_256": lambda: case_radius(256), "harris5": case_harris5,
         "odd_crop": case_odd_crop, "full_image": case_full_image}
RUN_KW = ("radius", "det", "fpb", "redetect_below", "stride", "bucket_threads", "bucket_size")


def check(got, imgs, frames, kw, lookahead):
    det, rb, radius = kw.get("det", tc.DEFAULT), kw.get("redetect_below", 2000), kw.get("radius", 5)
    for f, (image, pts, ages) in enumerate(frames):
        img = imgs[image]
        h, w = img.shape
        want_p, want_a, n_new = tc.expected_bucketed(img, pts, ages, radius, det, rb, kw.get("bucket_size", 0), kw.get("fpb", 1))
        g = got[f]
        assert g["overflow"] == 0 and g["n_new"] == n_new and g["n"] == len(want_p), (f, g["n"], g["n_new"], n_new)
        assert np.array_equal(g["pts"], want_p) and np.array_equal(g["ages"], want_a), f
        assert g["detect"] == (1 if len(pts) < rb else 0)
        if g["detect"]:
            assert np.array_equal(g["plane"], cm.ref_disc_mask(w, h, pts, radius)), (f, "the plane against the header's disc mask")
            assert g["max_key"] == g["body_key"], (f, hex(g["max_key"]), hex(g["body_key"]))
            assert (g["max_key"] == 0) == (not g["plane"].any())
        else:   # a frame that does not detect again: no plane, candidate or select pass -- and inline no map pass either
            assert g["plane_touched"] == 0 and g["cand_touched"] == 0 and g["n_cand"] == 0 and g["max_key"] == 0
            assert g["map_touched"] == (1 if lookahead else 0)


@pytest.mark.parametrize("lookahead", [False, True], ids=["inline", "lookahead"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_masked_frames_form_and_bucketing(name, lookahead):
    imgs, frames, kw = CASES[name]()
    check(tc.emu_run(imgs, frames, lookahead=lookahead, **kw), imgs, frames, kw, lookahead)


def test_case_premises():
    """the cases are about what they name: the all-zero mask, a whole-image disc, a mask that changes the list"""
    imgs, frames, kw = case_all_zero_mask()
    assert not cm.ref_disc_mask(32, 32, frames[0][1], 10).any() and tc.expected_bucketed(imgs[0], frames[0][1], frames[0][2], 10)[2] == 0
    imgs, frames, kw = case_radius(256)
    assert not cm.ref_disc_mask(64, 48, frames[0][1], 256).any()
    imgs, frames, kw = case_radius(0)
    assert (cm.ref_disc_mask(64, 48, frames[0][1], 0) == 0).sum() == 12
    for make in (case_two_images, case_harris5, case_odd_crop, case_skipped_points):
        imgs, frames, kw = make()
        image, pts, _ = frames[0]
        det = kw.get("det", tc.DEFAULT)
        a, b = tc.ref_topup_corners(imgs[image], pts, kw.get("radius", 5), det), dc.ref_corners(imgs[image], **det)
        assert a.shape != b.shape or not np.array_equal(a, b), make.__name__
    imgs, frames, kw = case_empty_carried()
    assert tc.expected_bucketed(imgs[0], *tc.EMPTY, 5)[0].tobytes() == dc.expected_bucketed(imgs[0], *tc.EMPTY)[0].tobytes()


def overflow_case():
    flat = np.full((48, 64), 90, np.uint8)
    flat[20:24, 30:34] = 200                       # four corners of one square: a handful of candidates
    kept = np.array([(3.0, 3.0), (60.0, 44.0)], np.float32)   # away from the square, and too few to bring the crop's list under 32
    return [tc.crop(tc.CROP_BIG), flat], [(0, kept, np.zeros(2, np.int32)), (1, kept, np.zeros(2, np.int32))]


@pytest.mark.parametrize("lookahead", [False, True], ids=["inline", "lookahead"])
def test_candidate_overflow_under_a_mask(lookahead):
    """only ALLOWED maxima count against the capacity: beyond it the select pass reports lcap + 1 corners, which bucket_kernel's split
    form turns into bit 0 of the frame's overflow flag; the frame beside it, whose candidates fit, is complete"""
    imgs, frames = overflow_case()
    lcap = 32
    free = tc.emu_run(imgs, frames[:1])[0]
    assert free["n_cand"] > lcap and free["n_cand"] < dc.emu_run(imgs, [(0,) + tc.EMPTY])[0]["n_cand"]   # the mask took candidates away
    got = tc.emu_run(imgs, frames, lcap=lcap, out_cap=512, lookahead=lookahead)
    assert got[0]["n_cand"] == free["n_cand"] and got[0]["n_new"] == lcap + 1 and got[0]["overflow"] & 1
    want_p, want_a, n_new = tc.expected_bucketed(imgs[1], frames[1][1], frames[1][2], 5)
    assert 0 < n_new <= lcap and got[1]["overflow"] == 0 and got[1]["n_new"] == n_new
    assert np.array_equal(got[1]["pts"], want_p) and np.array_equal(got[1]["ages"], want_a)


def test_standalone_under_sanitizers(tmp_path):
    """every case but the full image once more (the two with several frames in both orders, the others in one), and the overflow
    case, in the ASan + UBSan program: exit status 0, no report, the same bytes"""
    for i, name in enumerate(sorted(CASES)):
        if name == "full_image":
            continue
        imgs, frames, kw = CASES[name]()
        for lookahead in ((False, True) if name in ("detect_flag", "odd_crop") else (bool(i & 1),)):   # (both orders where they differ most)
            d = tmp_path / ("%s_%d" % (name, lookahead))
            d.mkdir()
            check(tc.run_standalone(d, imgs, frames, lookahead=lookahead, **kw), imgs, frames, kw, lookahead)
    d = tmp_path / "overflow"
    d.mkdir()
    imgs, frames = overflow_case()
    got = tc.run_standalone(d, imgs, frames[:1], lcap=32, out_cap=512)
    assert got[0]["n_new"] == 33 and got[0]["overflow"] & 1
