"""The frame loop with the Shi-Tomasi detector (include/vo_detector.h, vodet_*) on the MI355X: vo_detect_bucket, VO_STAGE_DETECT of
vo_batch_run and the lock-step loop (look-ahead and inline detection) under VODET_SHI_TOMASI.

Expected side, never the code under test: goodFeaturesToTrack from the references (detector_cases.ref_corners: the reference's own
featureDetectionGoodFeaturesToTrack where oracle/_ref exists, tests/host_check/corners_ref.c / corners_response_ref.c otherwise),
appendNewFeatures' list rule and the oracle's bucketingFeatures; for everything behind the bucketed set the product's own existing
calls given those points, which the existing suite holds to the oracle.  Every comparison is identity.  Schedules are pinned."""
import ctypes as C

import numpy as np
import pytest

import context_modes_cases as cc
import corners_scale as cs
import detector_cases as dc

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def pinned(ctx, prepare=0):
    ctx.set_schedule(pose_waves=2, pose_streams=1, prepare=prepare, epnp_wide_frames=4)
    return ctx


@pytest.fixture()
def ctx(volib):
    c = pinned(volib.Context(0, 480, 160, 4096, 4))
    c.set_detector("shi_tomasi")
    yield c
    c.close()


def same_bucketed(got, want, what):
    assert len(got[0]) == len(want[0]) and np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1]), (what, len(got[0]), len(want[0]))


def images(small_seq):
    L0 = small_seq["L"][0]
    return {"L0": L0, "big": np.ascontiguousarray(L0[dc.CROP_BIG]), "small": np.ascontiguousarray(L0[dc.CROP_SMALL])}


# ---- 1. vo_detect_bucket ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["L0", "big", "small"])
def test_detect_bucket_identity(ctx, small_seq, name):
    img = images(small_seq)[name]
    h, w = img.shape
    carried = dc.carried_set(w, h, 40, 5)
    for fpb in (1, 4):
        same_bucketed(ctx.detect_bucket(img, *dc.EMPTY, features_per_bucket=fpb), dc.expected_bucketed(img, *dc.EMPTY, features_per_bucket=fpb),
                      (name, "empty", fpb))
        want = dc.expected_bucketed(img, *carried, features_per_bucket=fpb)
        assert want[2] > 0
        same_bucketed(ctx.detect_bucket(img, *carried, features_per_bucket=fpb), want, (name, "carried + surplus ages", fpb))
    # a carried set of redetect_below points: no detection, bucketing alone
    want = dc.expected_bucketed(img, *carried, redetect_below=40)
    assert want[2] == 0
    same_bucketed(ctx.detect_bucket(img, *carried, redetect_below=40), want, (name, "no detection"))
    # a view whose rows are further apart than the width
    same_bucketed(ctx.detect_bucket(cc.padded(img), *carried), dc.expected_bucketed(img, *carried), (name, "strided"))


def test_detect_bucket_on_the_kept_left_image(ctx, small_seq, small_world):
    """img == NULL after a vo_track_frame: the left image of the pair the call kept, which is what FAST would read"""
    s = small_seq
    P_l, P_r = small_world.proj_matrices()
    ctx.track_frame(s["L"][0], s["R"][0], s["L"][1], s["R"][1], s["pts"][0], P_l, P_r)
    carried = dc.carried_set(480, 160, 40, 5)
    want = dc.expected_bucketed(s["L"][1], *carried)
    assert not np.array_equal(want[0], dc.expected_bucketed(s["L"][0], *carried)[0])
    same_bucketed(ctx.detect_bucket(None, *carried), want, "kept pair")


# ---- 2. parameters ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("det", [dc.FEW, dc.HARRIS5], ids=["50-0.05-10", "block5-harris"])
def test_parameters_reach_the_detector(ctx, small_seq, det):
    ctx.set_detector("shi_tomasi", **det)
    assert ctx.get_detector() == dict(det, detector="shi_tomasi")
    for name in ("L0", "big"):
        img = images(small_seq)[name]
        h, w = img.shape
        carried = dc.carried_set(w, h, 12, 2, seed=8)
        want = dc.expected_bucketed(img, *carried, det=det, features_per_bucket=2)
        assert not np.array_equal(want[0], dc.expected_bucketed(img, *carried, features_per_bucket=2)[0])   # the parameters decide
        same_bucketed(ctx.detect_bucket(img, *carried, features_per_bucket=2), want, name)


# ---- 3. VO_STAGE_DETECT -------------------------------------------------------------------------------------------------------
def test_batch_detect_stage(ctx, volib, small_seq, small_world):
    """two frames, the first of which carries redetect_below points and does not detect again: the bucketed sets against the
    reference, and everything behind them against the same run on those points set by vo_batch_set_points"""
    s = small_seq
    P_l, P_r = small_world.proj_matrices()
    h, w = s["L"][0].shape
    ctx.batch_configure(6, w, h, 2)
    for k in range(3):
        ctx.batch_upload_image(2 * k, s["L"][k])
        ctx.batch_upload_image(2 * k + 1, s["R"][k])
    ctx.batch_set_quads([[0, 1, 2, 3], [2, 3, 4, 5]])
    carried = [(s["pts"][0][:40], np.arange(45, dtype=np.int32) % 13), dc.EMPTY]
    for f, (p, a) in enumerate(carried):
        ctx.batch_set_features(f, p, a)
    ctx.batch_set_detect_params(features_per_bucket=2, redetect_below=40)
    ctx.batch_set_projection(P_l, P_r)
    ctx.batch_run(volib.STAGE_ALL | volib.STAGE_DETECT)
    ctx.batch_sync()
    want = [dc.expected_bucketed(s["L"][f], p, a, redetect_below=40, features_per_bucket=2) for f, (p, a) in enumerate(carried)]
    assert want[0][2] == 0 and want[1][2] > 1000
    got = []
    for f in range(2):
        same_bucketed(ctx.batch_get_features(f), want[f], ("frame", f))
        got.append((ctx.batch_get_filtered(f), ctx.batch_get_pose(f)))
    for f in range(2):
        ctx.batch_set_points(f, want[f][0])
    ctx.batch_run(volib.STAGE_ALL)
    ctx.batch_sync()
    for f in range(2):
        fil, pose = ctx.batch_get_filtered(f), ctx.batch_get_pose(f)
        assert len(fil["l1"]) > 10 or f == 0
        for k in ("l0", "r0", "l1", "r1", "xyz", "keep_idx", "keep_idx_circ"):
            assert got[f][0][k].tobytes() == fil[k].tobytes(), (f, k)
        assert got[f][1]["status"] == pose["status"] and got[f][1]["rvec"].tobytes() == pose["rvec"].tobytes()
        assert got[f][1]["tvec"].tobytes() == pose["tvec"].tobytes() and np.array_equal(got[f][1]["inliers"], pose["inliers"])


# ---- 4. the lock-step loop ----------------------------------------------------------------------------------------------------
PLAN_FULL = [0, 1, 2, 3, 4]          # the frame a sequence pushes in each step
PLAN_PAUSED = [0, 1, None, 2, 3]     # no pair in step 2: the sequence pauses, and restarts its image pair with frame 2
_mirror = {}


def mirror(volib, plan):
    """StereoOdometry(detector="shi_tomasi") fed the pairs of `plan`; a pause drops its previous pair as the loop does (the carried
    features and the pose stay).  Once per plan"""
    from visual_odom_amd import odometry
    key = tuple(plan)
    if key not in _mirror:
        world, L, R = dc.world_frames()
        P_l, P_r = world.proj_matrices()
        vo = odometry.StereoOdometry(P_l, P_r, max_w=480, max_h=160, keep_pair=False, detector="shi_tomasi", features_per_bucket=1)
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
@pytest.mark.parametrize("n_seq", [2, 1])
def test_lock_step_loop_equals_the_synchronous_loop(volib, n_seq, ring, prepare):
    from visual_odom_amd import odometry
    world, L, R = dc.world_frames()
    P_l, P_r = world.proj_matrices()
    plans = [PLAN_FULL, PLAN_PAUSED][:n_seq]
    ctx = pinned(volib.Context(0, 480, 160, 4096, n_seq), prepare)
    try:
        ms = odometry.MultiSequenceOdometry(P_l, P_r, n_seq, 480, 160, ring=ring, max_steps=8, ctx=ctx, detector="shi_tomasi", features_per_bucket=1)
        assert ctx.get_schedule()["prepare"] == prepare   # look-ahead detection on the prepare stream, or inline detection
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


def test_the_loop_follows_the_detector(volib):
    """the premise of the test above on the device: the Shi-Tomasi loop's log differs from the FAST loop's"""
    from visual_odom_amd import odometry
    world, L, R = dc.world_frames()
    P_l, P_r = world.proj_matrices()
    vo = odometry.StereoOdometry(P_l, P_r, max_w=480, max_h=160, keep_pair=False, features_per_bucket=1)
    try:
        pinned(vo.ctx)
        for k in PLAN_FULL:
            vo.process(L[k], R[k])
        fast = [r["n_bucketed"] for r in vo.log]
    finally:
        vo.close()
    shi = [r["n_bucketed"] for r in mirror(volib, PLAN_FULL)["log"]]
    assert len(fast) == len(shi) == 4 and all(a != b for a, b in zip(fast, shi)), (fast, shi)


# ---- 5. state -----------------------------------------------------------------------------------------------------------------
def test_fast_again_returns_the_bytes_of_a_fresh_context(ctx, volib, small_seq):
    img = small_seq["L"][0]
    carried = dc.carried_set(480, 160, 40, 5)
    fresh = pinned(volib.Context(0, 480, 160, 4096, 4))
    try:
        want = fresh.detect_bucket(img, *carried, features_per_bucket=2)
    finally:
        fresh.close()
    shi = ctx.detect_bucket(img, *carried, features_per_bucket=2)
    ctx.set_detector("fast")
    got = ctx.detect_bucket(img, *carried, features_per_bucket=2)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    assert shi[0].tobytes() != want[0].tobytes()


def test_set_params_inside_the_loop_is_refused(ctx, volib):
    ctx.seq_configure(1, 480, 160, 2, 4)
    before = ctx.get_detector()
    with pytest.raises(volib.VoError) as e:
        ctx.set_detector("fast")
    assert e.value.code == volib.VO_ERR_STATE and ctx.get_detector() == before


def test_bad_parameters_change_nothing(ctx, volib):
    lib = volib.load()
    before = ctx.get_detector()
    for kw in (dict(quality_level=0.0), dict(min_distance=-1.0), dict(max_corners=-1), dict(min_distance=257.0), dict(block_size=4), dict(k=float("nan"))):
        with pytest.raises(volib.VoError) as e:
            ctx.set_detector("shi_tomasi", **kw)
        assert e.value.code == volib.VO_ERR_ARG, kw
    prm = volib.VoDetParams()
    lib.vodet_default_params(C.byref(prm))
    prm.detector = 7
    assert lib.vodet_set_params(ctx.h, C.byref(prm)) == volib.VO_ERR_ARG and b"detector" in lib.vo_last_error(ctx.h)
    assert ctx.get_detector() == before
    assert lib.vodet_set_params(ctx.h, None) == 0 and ctx.get_detector() == dict(dc.DEFAULT, detector="fast")   # NULL: the defaults


def test_the_detector_calls_beside_the_frame_path(ctx, volib, small_seq):
    """the frame path runs in vocorn_*'s buffers: a later vocorn_batch_get answers VO_ERR_STATE, never another run's corners;
    vocorn_detect afterwards is what it was"""
    s = small_seq
    h, w = s["L"][0].shape
    ctx.batch_configure(4, w, h, 1)
    for i, img in enumerate((s["L"][0], s["R"][0], s["L"][1], s["R"][1])):
        ctx.batch_upload_image(i, img)
    ctx.corners_batch_run(0, 2)
    assert np.array_equal(ctx.corners_batch_get(0)[0], dc.ref_corners(s["L"][0]))
    ctx.batch_set_quads([[0, 1, 2, 3]])
    ctx.batch_set_features(0, *dc.EMPTY)
    ctx.batch_run(volib.STAGE_DETECT)
    ctx.batch_sync()
    same_bucketed(ctx.batch_get_features(0), dc.expected_bucketed(s["L"][0], *dc.EMPTY), "the stage itself")
    with pytest.raises(volib.VoError) as e:
        ctx.corners_batch_get(0)
    assert e.value.code == volib.VO_ERR_STATE
    assert np.array_equal(ctx.good_features_to_track(s["L"][1]), dc.ref_corners(s["L"][1]))
    ctx.detect_bucket(s["L"][0], *dc.EMPTY)
    assert np.array_equal(ctx.good_features_to_track(s["L"][1], max_corners=50, quality_level=0.05, min_distance=10.0),
                          dc.ref_corners(s["L"][1], 50, 0.05, 10.0))


# ---- 6. capacity --------------------------------------------------------------------------------------------------------------
def test_capacity(volib):
    """a context whose corner-list capacity is 16 384: the 16 384-candidate image runs complete, one candidate more is
    VO_ERR_OVERFLOW with the caller's arrays untouched"""
    full = next(c for c in cs.SCALE_CASES if c.name == "full-list-md5")
    over = next(c for c in cs.SCALE_CASES if c.name == "one-over-md0")
    assert cs.premise(full)[2] == cs.CAPACITY and cs.premise(over)[2] == cs.CAPACITY + 1
    h, w = full.img.shape
    ctx = pinned(volib.Context(0, w, h, 4096, 1))
    try:
        ctx.set_detector("shi_tomasi", max_corners=0)
        want = dc.expected_bucketed(full.img, *dc.EMPTY, det=dict(dc.DEFAULT, max_corners=0), features_per_bucket=4)
        assert want[2] == 676
        same_bucketed(ctx.detect_bucket(full.img, *dc.EMPTY, features_per_bucket=4), want, "full list")
        lib = volib.load()
        p_io = np.full((4096, 2), -3.0, np.float32)
        a_io = np.full(4096, -3, np.int32)
        n_pts, n_ages = C.c_int(0), C.c_int(0)
        img = np.ascontiguousarray(over.img)
        rc = lib.vo_detect_bucket(ctx.h, img.ctypes.data_as(C.c_void_p), w, h, w, None, p_io.ctypes.data_as(C.c_void_p), C.byref(n_pts),
                                  a_io.ctypes.data_as(C.c_void_p), C.byref(n_ages), 4096)
        assert rc == volib.VO_ERR_OVERFLOW and b"nothing was written" in lib.vo_last_error(ctx.h)
        assert (p_io == -3.0).all() and (a_io == -3).all() and n_pts.value == 0 and n_ages.value == 0
        same_bucketed(ctx.detect_bucket(full.img, *dc.EMPTY, features_per_bucket=4), want, "after the refusal")
    finally:
        ctx.close()


# ---- 7. a rectifying colour context -------------------------------------------------------------------------------------------
def test_rectifying_bgr_context_reads_the_image_fast_reads(volib, orc, small_seq, small_world):
    """convert, remap through the LEFT maps, then the detector -- the image the FAST path of the same call reads"""
    maps = cc.m_maps(small_world)
    raw, gray, _ = cc.encode(small_seq["L"][0], cc.BGR8, 71)
    rect = cc.remapped("detector-bgr-L0", gray, maps, 0)
    carried = dc.carried_set(480, 160, 40, 5)
    ctx = pinned(volib.Context(0, 480, 160, 4096, 1))
    try:
        ctx.set_params(rectify=maps, input_format=cc.BGR8)
        fast = orc.fast_detect(rect, 20, True)
        want_fast = orc.bucketing_features(160, 480, np.vstack([carried[0], fast]), np.concatenate([carried[1], np.zeros(len(fast), np.int32)]), 16, 1)
        same_bucketed(ctx.detect_bucket(raw, *carried), want_fast, "FAST")
        ctx.set_detector("shi_tomasi")
        want = dc.expected_bucketed(rect, *carried)
        assert not np.array_equal(want[0], dc.expected_bucketed(gray, *carried)[0])   # the unrectified image gives another set
        same_bucketed(ctx.detect_bucket(raw, *carried), want, "Shi-Tomasi")
    finally:
        ctx.close()
