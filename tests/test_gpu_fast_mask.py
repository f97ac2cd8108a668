"""cv::FAST under a mask (include/vo_fast_mask.h, vofm_*) on the MI355X: vofm_detect and vofm_replenish, and the record VOFM_CARRIED in
vo_detect_bucket, VO_STAGE_DETECT of vo_batch_run and the lock-step loop (the unmasked list as look-ahead with the discs and the filter
in the step, and the inline detection) under VODET_FAST.

Expected side, never the code under test: fast_mask_cases.py's composition -- the oracle's cv::FAST on the unmasked image,
runByPixelsMask in numpy, the header's disc mask (corners_mask_cases.ref_disc_mask), appendNewFeatures' list rule and the oracle's
bucketingFeatures; for the lock-step loop the synchronous loop over vo_detect_bucket + vo_track_frame, which the tests here hold to
that composition.  Every comparison is identity.  Schedules are pinned."""
import ctypes as C

import numpy as np
import pytest

import context_modes_cases as cc
import corners_mask_cases as cm
import detector_cases as dc
import fast_mask_cases as fm
from test_gpu_detector import PLAN_FULL, PLAN_PAUSED, bits, pinned, same_bucketed

pytestmark = pytest.mark.gpu


@pytest.fixture()
def ctx(volib):
    c = pinned(volib.Context(0, 480, 160, 4096, 4))
    c.set_fast_topup(radius=5)
    yield c
    c.close()


def images():
    return {"L0": fm.L0(), "big": fm.crop(fm.CROP_BIG), "small": fm.crop(fm.CROP_SMALL), "odd": fm.crop(fm.CROP_ODD)}


def carried_sets(img):
    h, w = img.shape
    every = fm.every_nth(img, 40)
    forty = fm.carried_set(w, h, 40, 5)      # 40 carried with 45 ages
    return {"empty": fm.EMPTY, "every 40th corner": every, "40 carried with 45 ages": forty}


def same_list(got, want, what):
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), (what, len(got), len(want))


# ---- 1. vofm_detect, vofm_replenish -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["L0", "big", "small", "odd"])
def test_detect_under_masks(ctx, name):
    img = images()[name]
    h, w = img.shape
    rng = np.random.default_rng(5)
    for what, carried in carried_sets(img).items():
        for radius in (0, 5, 10):
            mask = cm.ref_disc_mask(w, h, carried[0], radius)
            same_list(ctx.fast_detect_masked(img, mask), fm.ref_masked(img, mask), (name, what, radius))
            same_list(ctx.fast_replenish(img, carried[0], radius), fm.ref_masked(img, mask), (name, what, radius, "replenish"))
    mask = (rng.integers(0, 3, (h, w)) * rng.integers(1, 256, (h, w))).astype(np.uint8)   # a third zeros, any non-zero byte allows
    want = fm.ref_masked(img, mask)
    assert 0 < len(want) < len(fm.ref_fast(img))
    same_list(ctx.fast_detect_masked(img, mask), want, (name, "random bytes"))
    same_list(ctx.fast_detect_masked(cc.padded(img), mask), want, (name, "padded image"))
    same_list(ctx.fast_detect_masked(img, cc.padded(mask)), want, (name, "padded mask"))
    same_list(ctx.fast_detect_masked(img, mask, threshold=35, nonmax=False), fm.ref_masked(img, mask, 35, False), (name, "threshold, nonmax"))
    assert len(ctx.fast_detect_masked(img, np.zeros((h, w), np.uint8))) == 0
    # mask == NULL is vo_fast_detect
    assert ctx.fast_detect_masked(img, None).tobytes() == ctx.fast_detect(img).tobytes() == fm.ref_fast(img).tobytes()


def test_detect_with_a_small_cap(ctx, volib):
    """cap smaller than the result: the first cap corners are written, *n_out is the full count"""
    img = fm.L0()
    h, w = img.shape
    mask = cm.ref_disc_mask(w, h, fm.every_nth(img)[0], 5)
    want = fm.ref_masked(img, mask)
    lib = volib.load()
    out = np.full((50, 2), -3.0, np.float32)
    n = C.c_int(0)
    rc = lib.vofm_detect(ctx.h, img.ctypes.data_as(C.c_void_p), w, h, w, 20, 1, mask.ctypes.data_as(C.c_void_p), w, out.ctypes.data_as(C.c_void_p), 40,
                         C.byref(n))
    assert rc == 0 and n.value == len(want) == 1603 - 118
    assert np.array_equal(out[:40], want[:40]) and (out[40:] == -3.0).all()
    rc = lib.vofm_detect(ctx.h, img.ctypes.data_as(C.c_void_p), w, h, w, 20, 1, mask.ctypes.data_as(C.c_void_p), w, None, 0, C.byref(n))
    assert rc == 0 and n.value == len(want)


def test_bad_calls(ctx, volib):
    """the table of test_fast_mask_abi.py with a context: the documented code, and nothing changed"""
    lib = volib.load()
    img, mask = fm.crop(fm.CROP_BIG), np.full((48, 64), 255, np.uint8)
    pi, pm = img.ctypes.data_as(C.c_void_p), mask.ctypes.data_as(C.c_void_p)
    out = np.full((100, 2), -3.0, np.float32)
    po = out.ctypes.data_as(C.c_void_p)
    n = C.c_int(-9)
    kept = np.zeros((8200, 2), np.float32)
    pk = kept.ctypes.data_as(C.c_void_p)
    E = volib.VO_ERR_ARG
    assert lib.vofm_detect(ctx.h, pi, 64, 48, 64, 20, 1, None, 64, po, 100, C.byref(n)) == E and b"stride" in lib.vo_last_error(ctx.h)
    assert lib.vofm_detect(ctx.h, pi, 64, 48, 64, 20, 1, pm, 63, po, 100, C.byref(n)) == E and b"stride" in lib.vo_last_error(ctx.h)
    assert lib.vofm_detect(ctx.h, pi, 64, 48, 63, 20, 1, pm, 64, po, 100, C.byref(n)) == E
    assert lib.vofm_detect(ctx.h, pi, 64, 48, 64, 20, 1, pm, 64, po, 100, None) == E
    for radius in (-1, 257):
        assert lib.vofm_replenish(ctx.h, pi, 64, 48, 64, 20, 1, pk, 3, radius, po, 100, C.byref(n)) == E and b"radius" in lib.vo_last_error(ctx.h)
    assert lib.vofm_replenish(ctx.h, pi, 64, 48, 64, 20, 1, pk, 4097, 5, po, 100, C.byref(n)) == E and b"n_kept" in lib.vo_last_error(ctx.h)
    assert lib.vofm_replenish(ctx.h, pi, 64, 48, 64, 20, 1, None, 3, 5, po, 100, C.byref(n)) == E
    assert n.value == -9 and (out == -3.0).all()
    before = ctx.get_fast_topup()
    for radius in (-1, 257):
        with pytest.raises(volib.VoError) as e:
            ctx.set_fast_topup(radius=radius)
        assert e.value.code == E and b"radius" in lib.vo_last_error(ctx.h)
    prm = volib.VoFmParams(7, 5)
    assert lib.vofm_set_params(ctx.h, C.byref(prm)) == E and b"mode" in lib.vo_last_error(ctx.h)
    assert ctx.get_fast_topup() == before == dict(radius=5, mode="carried")
    assert lib.vofm_set_params(ctx.h, None) == 0 and ctx.get_fast_topup() == dict(radius=5, mode="off")   # NULL: the defaults
    assert lib.vofm_get_mask(ctx.h, 0, None, 64) == E and lib.vofm_get_mask(ctx.h, 0, pm, -1) == E


# ---- 2. vo_detect_bucket ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["L0", "big", "small", "odd"])
def test_detect_bucket_identity(ctx, volib, name):
    img = images()[name]
    h, w = img.shape
    sets = carried_sets(img)
    for radius in (0, 5, 10):
        ctx.set_fast_topup(radius=radius)
        assert ctx.get_fast_topup() == dict(radius=radius, mode="carried")
        for what, carried in sets.items():
            want = fm.expected_bucketed(img, *carried, radius, features_per_bucket=4)
            same_bucketed(ctx.detect_bucket(img, *carried, features_per_bucket=4), want, (name, what, radius))
            assert np.array_equal(ctx.fast_topup_mask(0, w, h), cm.ref_disc_mask(w, h, carried[0], radius)), (name, what, radius)
    # the empty carried set is the unmasked call, byte for byte
    same_bucketed(ctx.detect_bucket(img, *fm.EMPTY), fm.expected_bucketed(img, *fm.EMPTY, None), (name, "unmasked"))
    # a carried set of redetect_below points: no detection, bucketing alone, and no plane to fetch
    carried = sets["40 carried with 45 ages"]
    want = fm.expected_bucketed(img, *carried, 10, redetect_below=40)
    assert want[2] == 0
    same_bucketed(ctx.detect_bucket(img, *carried, redetect_below=40), want, (name, "no detection"))
    with pytest.raises(volib.VoError) as e:
        ctx.fast_topup_mask(0, w, h)
    assert e.value.code == volib.VO_ERR_STATE
    # a view whose rows are further apart than the width
    same_bucketed(ctx.detect_bucket(cc.padded(img), *carried), fm.expected_bucketed(img, *carried, 10), (name, "strided"))


def test_the_mask_decides(ctx):
    """the premises of test_fast_mask_ref.py on the device: 118 of L[0]'s 1 603 corners leave, and the bucketed set differs from the
    unmasked one at 1 and at 4 features per bucket"""
    img = fm.L0()
    carried = fm.every_nth(img, 40)
    for fpb in (1, 4):
        want = fm.expected_bucketed(img, *carried, 5, features_per_bucket=fpb)
        plain = fm.expected_bucketed(img, *carried, None, features_per_bucket=fpb)
        assert want[2] == 1603 - 118 and plain[2] == 1603 and want[0].tobytes() != plain[0].tobytes()
        same_bucketed(ctx.detect_bucket(img, *carried, features_per_bucket=fpb), want, fpb)


def test_the_all_zero_mask(ctx):
    small = fm.crop(fm.CROP_SMALL)
    carried = fm.carried_set(32, 32, 40, 5)
    ctx.set_fast_topup(radius=10)
    want = fm.expected_bucketed(small, *carried, 10)
    assert want[2] == 0
    same_bucketed(ctx.detect_bucket(small, *carried), want, "0 corners and no error")
    assert not ctx.fast_topup_mask(0, 32, 32).any()


def test_on_the_kept_left_image(ctx, small_seq, small_world):
    """img == NULL after a vo_track_frame: the left image of the pair the call kept"""
    s = small_seq
    P_l, P_r = small_world.proj_matrices()
    ctx.track_frame(s["L"][0], s["R"][0], s["L"][1], s["R"][1], s["pts"][0], P_l, P_r)
    carried = fm.carried_set(480, 160, 40, 5)
    want = fm.expected_bucketed(s["L"][1], *carried, 5)
    assert not np.array_equal(want[0], fm.expected_bucketed(s["L"][0], *carried, 5)[0])
    same_bucketed(ctx.detect_bucket(None, *carried), want, "kept pair")
    mask = cm.ref_disc_mask(480, 160, carried[0], 7)
    same_list(ctx.fast_detect_masked(None, mask), fm.ref_masked(s["L"][1], mask), "vofm_detect on the kept image")


# ---- 3. VO_STAGE_DETECT -------------------------------------------------------------------------------------------------------
def test_batch_detect_stage(ctx, volib, small_seq):
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
    want = [fm.expected_bucketed(s["L"][f], p, a, 5, redetect_below=40, features_per_bucket=2) for f, (p, a) in enumerate(carried)]
    assert want[0][2] == 0 and want[1][2] > 500
    assert not np.array_equal(want[1][0], fm.expected_bucketed(s["L"][1], *carried[1], None, redetect_below=40, features_per_bucket=2)[0])
    for f in range(2):
        same_bucketed(ctx.batch_get_features(f), want[f], ("frame", f))
    assert np.array_equal(ctx.fast_topup_mask(1, w, h), cm.ref_disc_mask(w, h, carried[1][0], 5))
    with pytest.raises(volib.VoError) as e:
        ctx.fast_topup_mask(0, w, h)   # frame 0 did not detect again
    assert e.value.code == volib.VO_ERR_STATE


# ---- 4. the lock-step loop ----------------------------------------------------------------------------------------------------
_mirror = {}


def mirror(volib, plan, fast_topup_radius=5):
    """StereoOdometry(fast_topup_radius=...) fed the pairs of `plan`; a pause drops its previous pair as the loop does.  Once per plan"""
    from visual_odom_amd import odometry
    key = (tuple(plan), fast_topup_radius)
    if key not in _mirror:
        world, L, R = dc.world_frames()
        P_l, P_r = world.proj_matrices()
        vo = odometry.StereoOdometry(P_l, P_r, max_w=480, max_h=160, keep_pair=False, fast_topup_radius=fast_topup_radius, features_per_bucket=1)
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
        ms = odometry.MultiSequenceOdometry(P_l, P_r, 2, 480, 160, ring=ring, max_steps=8, ctx=ctx, fast_topup_radius=5, features_per_bucket=1)
        assert ctx.get_schedule()["prepare"] == prepare and ctx.get_fast_topup() == dict(radius=5, mode="carried")
        assert ctx.get_detector()["detector"] == "fast"
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


def test_the_loop_follows_the_mask(volib):
    """the synchronous loop's bucketed counts equal the unmasked FAST loop's in frame 0 -- nothing is carried in -- and differ from
    frame 1 on"""
    top = [r["n_bucketed"] for r in mirror(volib, PLAN_FULL)["log"]]
    plain = [r["n_bucketed"] for r in mirror(volib, PLAN_FULL, fast_topup_radius=False)["log"]]
    assert top == [274, 279, 282, 290] and plain == [274, 280, 287, 293], (top, plain)
    assert top[0] == plain[0] and all(a != b for a, b in zip(top[1:], plain[1:])), (top, plain)


# ---- 5. state -----------------------------------------------------------------------------------------------------------------
def test_off_again_returns_the_bytes_of_a_fresh_context(ctx, volib):
    img = fm.L0()
    carried = fm.carried_set(480, 160, 40, 5)
    fresh = pinned(volib.Context(0, 480, 160, 4096, 4))
    try:
        want = fresh.detect_bucket(img, *carried, features_per_bucket=2)
        want_fast = fresh.fast_detect(img)
    finally:
        fresh.close()
    on = ctx.detect_bucket(img, *carried, features_per_bucket=2)
    ctx.set_fast_topup(mode="off")
    assert ctx.get_fast_topup() == dict(radius=5, mode="off")
    got = ctx.detect_bucket(img, *carried, features_per_bucket=2)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    assert on[0].tobytes() != want[0].tobytes()
    assert ctx.fast_detect(img).tobytes() == want_fast.tobytes()
    with pytest.raises(volib.VoError) as e:
        ctx.fast_topup_mask(0, 480, 160)   # no masked detection since the record changed
    assert e.value.code == volib.VO_ERR_STATE


def test_under_shi_tomasi_the_record_changes_nothing(volib):
    img = fm.L0()
    carried = fm.carried_set(480, 160, 40, 5)
    c = pinned(volib.Context(0, 480, 160, 4096, 1))
    try:
        c.set_detector("shi_tomasi")
        want = c.detect_bucket(img, *carried, features_per_bucket=2)
        c.set_fast_topup(radius=9)
        assert c.get_fast_topup() == dict(radius=9, mode="carried") and c.get_detector()["detector"] == "shi_tomasi"
        got = c.detect_bucket(img, *carried, features_per_bucket=2)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
        with pytest.raises(volib.VoError) as e:
            c.fast_topup_mask(0, 480, 160)
        assert e.value.code == volib.VO_ERR_STATE
    finally:
        c.close()


def test_votops_record_under_fast_still_changes_nothing(volib):
    img = fm.L0()
    carried = fm.carried_set(480, 160, 40, 5)
    c = pinned(volib.Context(0, 480, 160, 4096, 1))
    try:
        want = c.detect_bucket(img, *carried, features_per_bucket=2)
        c.set_topup(radius=9)
        assert c.get_fast_topup() == dict(radius=5, mode="off")
        got = c.detect_bucket(img, *carried, features_per_bucket=2)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
        same_bucketed(got, fm.expected_bucketed(img, *carried, None, features_per_bucket=2), "the unmasked composition")
    finally:
        c.close()


def test_set_params_inside_the_loop_is_refused(ctx, volib):
    ctx.seq_configure(1, 480, 160, 2, 4)
    before = ctx.get_fast_topup()
    for kw in (dict(mode="off"), dict(radius=7)):
        with pytest.raises(volib.VoError) as e:
            ctx.set_fast_topup(**kw)
        assert e.value.code == volib.VO_ERR_STATE and ctx.get_fast_topup() == before
    with pytest.raises(volib.VoError) as e:
        ctx.fast_topup_mask(0, 480, 160)
    assert e.value.code == volib.VO_ERR_STATE
    with pytest.raises(volib.VoError) as e:
        ctx.fast_detect_masked(fm.L0(), np.full((160, 480), 255, np.uint8))
    assert e.value.code == volib.VO_ERR_STATE


# ---- 6. capacity --------------------------------------------------------------------------------------------------------------
def test_overflow_of_the_unmasked_list(volib, orc):
    """FAST(1, no NMS) on noise finds more corners than the context's corner list holds (32 768): the capacity is judged on the
    unmasked list, whatever the mask leaves -- vofm_detect and vo_detect_bucket answer VO_ERR_OVERFLOW with nothing written; on an
    ordinary image the same context is complete"""
    rng = np.random.default_rng(4)
    noise = rng.integers(0, 256, (512, 1024), dtype=np.uint8)
    assert len(orc.fast_detect(noise, 1, False, cap=600000)) > 32768
    h, w = noise.shape
    mask = np.zeros((h, w), np.uint8)
    mask[:8] = 255                       # what the mask leaves would fit many times over
    ctx = pinned(volib.Context(0, 1024, 512, 4096, 1))
    try:
        lib = volib.load()
        out = np.full((40000, 2), -3.0, np.float32)
        n = C.c_int(-9)
        rc = lib.vofm_detect(ctx.h, noise.ctypes.data_as(C.c_void_p), w, h, w, 1, 0, mask.ctypes.data_as(C.c_void_p), w, out.ctypes.data_as(C.c_void_p), 40000,
                             C.byref(n))
        assert rc == volib.VO_ERR_OVERFLOW and b"nothing was written" in lib.vo_last_error(ctx.h)
        assert (out == -3.0).all() and n.value > 32768
        ctx.set_fast_topup(radius=256)
        p_io = np.full((4096, 2), -3.0, np.float32)
        a_io = np.full(4096, -3, np.int32)
        p_io[0] = (500.0, 250.0)
        a_io[0] = 0
        n_pts, n_ages = C.c_int(1), C.c_int(1)
        dp = volib.VoDetectParams(1, 0, 2000, 0, 1)
        rc = lib.vo_detect_bucket(ctx.h, noise.ctypes.data_as(C.c_void_p), w, h, w, C.byref(dp), p_io.ctypes.data_as(C.c_void_p), C.byref(n_pts),
                                  a_io.ctypes.data_as(C.c_void_p), C.byref(n_ages), 4096)
        assert rc == volib.VO_ERR_OVERFLOW and b"nothing was written" in lib.vo_last_error(ctx.h)
        assert (p_io[1:] == -3.0).all() and (a_io[1:] == -3).all() and n_pts.value == 1 and n_ages.value == 1
        img = fm.L0()
        carried = fm.every_nth(img, 40)
        ctx.set_fast_topup(radius=5)
        same_bucketed(ctx.detect_bucket(img, *carried), fm.expected_bucketed(img, *carried, 5), "under the capacity")
    finally:
        ctx.close()
