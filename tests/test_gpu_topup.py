"""The frame loop's top-up under a mask of the carried points (include/vo_topup.h, votop_*) on the MI355X: vo_detect_bucket,
VO_STAGE_DETECT of vo_batch_run and the lock-step loop (the map pass as look-ahead with the masked passes in the step, and the inline
detection) under VODET_SHI_TOMASI with VOTOP_CARRIED.

Expected side, never the code under test: topup_cases.py's composition -- the header's disc mask (corners_mask_cases.ref_disc_mask),
goodFeaturesToTrack under it (tests/host_check/corners_response_ref.c), appendNewFeatures' list rule and the oracle's
bucketingFeatures; for the lock-step loop the synchronous loop over vo_detect_bucket + vo_track_frame, which the tests here hold to
that composition.  Every comparison is identity.  Schedules are pinned."""
import ctypes as C

import numpy as np
import pytest

import context_modes_cases as cc
import corners_mask_cases as cm
import corners_response_cases as crc
import corners_scale as cs
import detector_cases as dc
import topup_cases as tc
from test_gpu_detector import PLAN_FULL, PLAN_PAUSED, bits, pinned, same_bucketed

pytestmark = pytest.mark.gpu


@pytest.fixture()
def ctx(volib):
    c = pinned(volib.Context(0, 480, 160, 4096, 4))
    c.set_detector("shi_tomasi")
    c.set_topup(radius=5)
    yield c
    c.close()


def images():
    return {"L0": tc.L0(), "big": tc.crop(tc.CROP_BIG), "small": tc.crop(tc.CROP_SMALL), "odd": tc.crop(tc.CROP_ODD)}


def with_ages(pts, surplus=3):
    return pts, (np.arange(len(pts) + surplus) % 13).astype(np.int32)


# ---- 1. vo_detect_bucket ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["L0", "big", "small", "odd"])
def test_detect_bucket_identity(ctx, name):
    img = images()[name]
    h, w = img.shape
    sets = {"empty": tc.EMPTY, "carried": tc.carried_set(w, h, 40, 5), "strongest": with_ages(tc.strongest(img, 8))}
    for radius in (0, 5, 10):
        ctx.set_topup(radius=radius)
        assert ctx.get_topup() == dict(radius=radius, mode="carried")
        for what, carried in sets.items():
            want = tc.expected_bucketed(img, *carried, radius, features_per_bucket=4)
            same_bucketed(ctx.detect_bucket(img, *carried, features_per_bucket=4), want, (name, what, radius))
            if len(carried[0]):   # the disc pass alone: the plane the call built
                assert np.array_equal(ctx.topup_mask(0, w, h), cm.ref_disc_mask(w, h, carried[0], radius)), (name, what, radius)
    # the empty carried set is the unmasked call, byte for byte
    same_bucketed(ctx.detect_bucket(img, *tc.EMPTY), dc.expected_bucketed(img, *tc.EMPTY), (name, "unmasked"))
    # a carried set of redetect_below points: no detection, bucketing alone, and no plane to fetch
    carried = sets["carried"]
    want = tc.expected_bucketed(img, *carried, 10, redetect_below=40)
    assert want[2] == 0
    same_bucketed(ctx.detect_bucket(img, *carried, redetect_below=40), want, (name, "no detection"))
    # a view whose rows are further apart than the width
    same_bucketed(ctx.detect_bucket(cc.padded(img), *carried), tc.expected_bucketed(img, *carried, 10), (name, "strided"))


def test_the_mask_decides(ctx):
    """the premises of test_topup_ref.py on the device: with the strongest corner carried the call finds MORE corners than unmasked"""
    img = tc.L0()
    carried = with_ages(tc.strongest(img, 1), 0)
    ctx.set_topup(radius=5)
    want = tc.expected_bucketed(img, *carried, 5, features_per_bucket=4)
    assert want[2] == 1054 and len(dc.ref_corners(img)) == 1016
    same_bucketed(ctx.detect_bucket(img, *carried, features_per_bucket=4), want, "strongest corner carried")


def test_the_all_zero_mask(ctx, volib):
    small = tc.crop(tc.CROP_SMALL)
    carried = tc.carried_set(32, 32, 40, 5)
    ctx.set_topup(radius=10)
    want = tc.expected_bucketed(small, *carried, 10)
    assert want[2] == 0
    same_bucketed(ctx.detect_bucket(small, *carried), want, "0 corners and no error")
    assert not ctx.topup_mask(0, 32, 32).any()


def test_detect_bucket_on_the_kept_left_image(ctx, small_seq, small_world):
    """img == NULL after a vo_track_frame: the left image of the pair the call kept, which is what FAST would read"""
    s = small_seq
    P_l, P_r = small_world.proj_matrices()
    ctx.track_frame(s["L"][0], s["R"][0], s["L"][1], s["R"][1], s["pts"][0], P_l, P_r)
    carried = tc.carried_set(480, 160, 40, 5)
    want = tc.expected_bucketed(s["L"][1], *carried, 5)
    assert not np.array_equal(want[0], tc.expected_bucketed(s["L"][0], *carried, 5)[0])
    same_bucketed(ctx.detect_bucket(None, *carried), want, "kept pair")


def test_parameters_reach_the_masked_call(ctx):
    img = tc.L0()
    carried = with_ages(tc.strongest(img, 1, tc.HARRIS5), 2)
    ctx.set_detector("shi_tomasi", **tc.HARRIS5)
    want = tc.expected_bucketed(img, *carried, 5, det=tc.HARRIS5, features_per_bucket=4)
    assert want[2] == 384
    same_bucketed(ctx.detect_bucket(img, *carried, features_per_bucket=4), want, "block 5, Harris")


# ---- 2. VO_STAGE_DETECT -------------------------------------------------------------------------------------------------------
def test_batch_detect_stage(ctx, volib, small_seq, small_world):
    """two frames, the first of which carries redetect_below points and does not detect again"""
    s = small_seq
    h, w = s["L"][0].shape
    ctx.batch_configure(6, w, h, 2)
    for k in range(3):
        ctx.batch_upload_image(2 * k, s["L"][k])
        ctx.batch_upload_image(2 * k + 1, s["R"][k])
    ctx.batch_set_quads([[0, 1, 2, 3], [2, 3, 4, 5]])
    carried = [(s["pts"][0][:40], np.arange(45, dtype=np.int32) % 13), (s["pts"][1][:25], np.arange(25, dtype=np.int32) % 13)]
    for f, (p, a) in enumerate(carried):
        ctx.batch_set_features(f, p, a)
    ctx.batch_set_detect_params(features_per_bucket=2, redetect_below=40)
    ctx.batch_run(volib.STAGE_DETECT)
    ctx.batch_sync()
    want = [tc.expected_bucketed(s["L"][f], p, a, 5, redetect_below=40, features_per_bucket=2) for f, (p, a) in enumerate(carried)]
    assert want[0][2] == 0 and want[1][2] > 500
    assert not np.array_equal(want[1][0], dc.expected_bucketed(s["L"][1], *carried[1], redetect_below=40, features_per_bucket=2)[0])
    for f in range(2):
        same_bucketed(ctx.batch_get_features(f), want[f], ("frame", f))
    assert np.array_equal(ctx.topup_mask(1, w, h), cm.ref_disc_mask(w, h, carried[1][0], 5))
    with pytest.raises(volib.VoError) as e:
        ctx.topup_mask(0, w, h)   # frame 0 did not detect again
    assert e.value.code == volib.VO_ERR_STATE


# ---- 3. the lock-step loop ----------------------------------------------------------------------------------------------------
_mirror = {}


def mirror(volib, plan, topup_radius=5):
    """StereoOdometry(detector="shi_tomasi", topup_radius=...) fed the pairs of `plan`; a pause drops its previous pair as the loop does.
    Once per plan"""
    from visual_odom_amd import odometry
    key = (tuple(plan), topup_radius)
    if key not in _mirror:
        world, L, R = dc.world_frames()
        P_l, P_r = world.proj_matrices()
        vo = odometry.StereoOdometry(P_l, P_r, max_w=480, max_h=160, keep_pair=False, detector="shi_tomasi", topup_radius=topup_radius,
                                     features_per_bucket=1)
        try:
            pinned(vo.ctx)
            for k in plan:
                if k is None:
                    vo.prev = None
                else:
                    vo.process(L[k], R[k])
            _mirror[key] = dict(points=vo.points.copy(), ages=vo.ages.copy(), pose=vo.frame_pose.copy(), log=list(vo.log))
        finally:
            vo.close()
    return _mirror[key]


@pytest.mark.parametrize("prepare", [1, 0], ids=["lookahead", "inline"])
@pytest.mark.parametrize("ring", [2, 3])
def test_lock_step_loop_equals_the_synchronous_loop(volib, ring, prepare):
    from visual_odom_amd import odometry
    world, L, R = dc.world_frames()
    P_l, P_r = world.proj_matrices()
    plans = [PLAN_FULL, PLAN_PAUSED]
    ctx = pinned(volib.Context(0, 480, 160, 4096, 2), prepare)
    try:
        ms = odometry.MultiSequenceOdometry(P_l, P_r, 2, 480, 160, ring=ring, max_steps=8, ctx=ctx, detector="shi_tomasi", topup_radius=5,
                                            features_per_bucket=1)
        assert ctx.get_schedule()["prepare"] == prepare and ctx.get_topup() == dict(radius=5, mode="carried")
        for step in range(5):
            for s, plan in enumerate(plans):
                if plan[step] is not None:
                    ms.push(s, L[plan[step]], R[plan[step]])
            ms.step()
        ms.sync()
        for s, plan in enumerate(plans):
            want = mirror(volib, plan)
            pts, ages, pose = ms.state(s)
            assert np.array_equal(bits(pts), bits(want["points"])) and np.array_equal(ages, want["ages"]), (s, len(pts), len(want["points"]))
            assert pose.tobytes() == want["pose"].tobytes(), (s, "frame_pose")
            log = ms.log(s)
            assert len(log) == len(want["log"]) == (4 if plan is PLAN_FULL else 2)
            for a, b in zip(log, want["log"]):
                assert a["overflow"] == 0 and (a["n_bucketed"], a["n_tracked"], a["n_inliers"]) == (b["n_bucketed"], b["n_tracked"], b["n_inliers"])
                assert a["rvec"].tobytes() == b["rvec"].tobytes() and a["tvec"].tobytes() == b["tvec"].tobytes() and a["integrated"] == b["integrated"]
    finally:
        ctx.close()


def test_the_loop_follows_the_top_up(volib):
    """the synchronous loop's bucketed counts are the reference loop's (test_topup_ref.py), equal to the unmasked Shi-Tomasi loop's
    in frame 0 -- nothing is carried in -- and different from frame 1 on"""
    top = [r["n_bucketed"] for r in mirror(volib, PLAN_FULL)["log"]]
    plain = [r["n_bucketed"] for r in mirror(volib, PLAN_FULL, topup_radius=False)["log"]]
    assert top == [283, 287, 287, 291], top
    assert top[0] == plain[0] and all(a != b for a, b in zip(top[1:], plain[1:])), (top, plain)


# ---- 4. state -----------------------------------------------------------------------------------------------------------------
def test_off_again_returns_the_bytes_of_a_fresh_shi_tomasi_context(ctx, volib):
    img = tc.L0()
    carried = tc.carried_set(480, 160, 40, 5)
    fresh = pinned(volib.Context(0, 480, 160, 4096, 4))
    try:
        fresh.set_detector("shi_tomasi")
        want = fresh.detect_bucket(img, *carried, features_per_bucket=2)
    finally:
        fresh.close()
    on = ctx.detect_bucket(img, *carried, features_per_bucket=2)
    ctx.set_topup(mode="off")
    assert ctx.get_topup() == dict(radius=5, mode="off")
    got = ctx.detect_bucket(img, *carried, features_per_bucket=2)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    assert on[0].tobytes() != want[0].tobytes()
    with pytest.raises(volib.VoError) as e:
        ctx.topup_mask(0, 480, 160)   # no masked detection since the record changed
    assert e.value.code == volib.VO_ERR_STATE


def test_under_fast_the_record_changes_nothing(volib):
    img = tc.L0()
    carried = tc.carried_set(480, 160, 40, 5)
    c = pinned(volib.Context(0, 480, 160, 4096, 1))
    try:
        want = c.detect_bucket(img, *carried, features_per_bucket=2)
        c.set_topup(radius=9)
        assert c.get_topup() == dict(radius=9, mode="carried") and c.get_detector()["detector"] == "fast"
        got = c.detect_bucket(img, *carried, features_per_bucket=2)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
        with pytest.raises(volib.VoError) as e:
            c.topup_mask(0, 480, 160)
        assert e.value.code == volib.VO_ERR_STATE
    finally:
        c.close()


def test_set_params_inside_the_loop_is_refused(ctx, volib):
    ctx.seq_configure(1, 480, 160, 2, 4)
    before = ctx.get_topup()
    for kw in (dict(mode="off"), dict(radius=7)):
        with pytest.raises(volib.VoError) as e:
            ctx.set_topup(**kw)
        assert e.value.code == volib.VO_ERR_STATE and ctx.get_topup() == before
    with pytest.raises(volib.VoError) as e:
        ctx.topup_mask(0, 480, 160)
    assert e.value.code == volib.VO_ERR_STATE


def test_bad_parameters_change_nothing(ctx, volib):
    lib = volib.load()
    before = ctx.get_topup()
    for radius in (-1, 257):
        with pytest.raises(volib.VoError) as e:
            ctx.set_topup(radius=radius)
        assert e.value.code == volib.VO_ERR_ARG and b"radius" in lib.vo_last_error(ctx.h)
    prm = volib.VoTopParams(7, 5)
    assert lib.votop_set_params(ctx.h, C.byref(prm)) == volib.VO_ERR_ARG and b"mode" in lib.vo_last_error(ctx.h)
    assert ctx.get_topup() == before
    assert lib.votop_set_params(ctx.h, None) == 0 and ctx.get_topup() == dict(radius=5, mode="off")   # NULL: the defaults


def test_the_detector_calls_beside_the_frame_path(ctx, volib, small_seq):
    """the frame path runs in vocorn_*'s buffers and keeps planes of its own: vocorn_*, vocmask_* and voresp_* are what they were"""
    s = small_seq
    h, w = s["L"][0].shape
    carried = tc.carried_set(w, h, 40, 5)
    ctx.batch_configure(4, w, h, 1)
    for i, img in enumerate((s["L"][0], s["R"][0], s["L"][1], s["R"][1])):
        ctx.batch_upload_image(i, img)
    ctx.corners_batch_run(0, 2)
    assert np.array_equal(ctx.corners_batch_get(0)[0], dc.ref_corners(s["L"][0]))
    ctx.batch_set_quads([[0, 1, 2, 3]])
    ctx.batch_set_features(0, *carried)
    ctx.batch_run(volib.STAGE_DETECT)
    ctx.batch_sync()
    same_bucketed(ctx.batch_get_features(0), tc.expected_bucketed(s["L"][0], *carried, 5), "the stage itself")
    with pytest.raises(volib.VoError) as e:
        ctx.corners_batch_get(0)
    assert e.value.code == volib.VO_ERR_STATE
    assert np.array_equal(ctx.good_features_to_track(s["L"][1]), dc.ref_corners(s["L"][1]))
    kept = carried[0][:9]
    assert np.array_equal(ctx.corner_disc_mask(w, h, kept, 7), cm.ref_disc_mask(w, h, kept, 7))
    ctx.detect_bucket(s["L"][0], *carried)
    assert np.array_equal(ctx.replenish_corners(s["L"][1], kept, 7), tc.ref_masked(s["L"][1], cm.ref_disc_mask(w, h, kept, 7)))
    same_bucketed(ctx.detect_bucket(s["L"][0], *carried), tc.expected_bucketed(s["L"][0], *carried, 5), "after the masked calls")
    assert np.array_equal(ctx.good_features_to_track(s["L"][1], block_size=5, use_harris=True), dc.ref_corners(s["L"][1], **tc.HARRIS5))


# ---- 5. capacity --------------------------------------------------------------------------------------------------------------
def test_masked_candidate_overflow(volib):
    """16 385 candidates on a context whose corner-list capacity is 16 384: under a mask that leaves them all the call is
    VO_ERR_OVERFLOW with the caller's arrays untouched; a disc over one of them brings the list under the capacity and the call is
    complete -- only allowed maxima count"""
    over = next(c for c in cs.SCALE_CASES if c.name == "one-over-md0")
    img = np.ascontiguousarray(over.img)
    h, w = img.shape
    det = dict(tc.DEFAULT, max_corners=0)
    aside = (np.array([[250.0, 120.0]], np.float32), np.zeros(1, np.int32))     # in the flat part: no candidate under the disc
    on_dot = (np.array([[200.0, 60.0]], np.float32), np.zeros(1, np.int32))     # over the isolated dot
    n_aside = crc.ref_detect(img, cm.ref_disc_mask(w, h, aside[0], 2), 0, 0.01, 5.0)[2]
    n_dot = crc.ref_detect(img, cm.ref_disc_mask(w, h, on_dot[0], 3), 0, 0.01, 5.0)[2]
    assert n_aside == cs.CAPACITY + 1 and 0 < n_dot <= cs.CAPACITY, (n_aside, n_dot)
    ctx = pinned(volib.Context(0, w, h, 4096, 1))
    try:
        ctx.set_detector("shi_tomasi", max_corners=0)
        lib = volib.load()
        ctx.set_topup(radius=2)
        p_io = np.full((4096, 2), -3.0, np.float32)
        a_io = np.full(4096, -3, np.int32)
        p_io[0] = aside[0][0]
        a_io[0] = 0
        n_pts, n_ages = C.c_int(1), C.c_int(1)
        rc = lib.vo_detect_bucket(ctx.h, img.ctypes.data_as(C.c_void_p), w, h, w, None, p_io.ctypes.data_as(C.c_void_p), C.byref(n_pts),
                                  a_io.ctypes.data_as(C.c_void_p), C.byref(n_ages), 4096)
        assert rc == volib.VO_ERR_OVERFLOW and b"nothing was written" in lib.vo_last_error(ctx.h)
        assert (p_io[1:] == -3.0).all() and (a_io[1:] == -3).all() and n_pts.value == 1 and n_ages.value == 1
        ctx.set_topup(radius=3)
        same_bucketed(ctx.detect_bucket(img, *on_dot, features_per_bucket=4), tc.expected_bucketed(img, *on_dot, 3, det=det, features_per_bucket=4),
                      "under the capacity")
    finally:
        ctx.close()
