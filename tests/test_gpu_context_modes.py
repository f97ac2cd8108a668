"""The flow calls (include/vo_flow.h, vo_flow_win.h, vo_flow_flags.h) and the corner calls (vo_corners.h, vo_corners_mask.h) on the
MI355X in a context with rectification maps (vo_params.rectify) and / or a colour or interleaved vo_params.input_format -- the
host layer's own code for those modes (capi_flow.hip: flow_sync_call's constant pair {0, 2, 0, 2}; capi_corners.hip:
corn_sync_image's plain upload; the image table's parity rule).

Every expected value is composed in tests/context_modes_cases.py from the project's CPU specification, in the order the headers
state: convert (test_gpu_ingest_formats.to_gray), remap (rectify_cases.remap_ref), then the checker's tracker or the detector's
reference.  Every comparison is BIT FOR BIT on every point.  tests/test_context_modes_premises.py shows on the CPU that each
expected answer differs from what the wrong side's maps, the unrectified image or the exchanged channels would give, so a routing
slip fails here.  Each test makes its own small context; schedules are pinned wherever a stereo call is made."""
import contextlib

import numpy as np
import pytest

import context_modes_cases as cc
import corners_mask_cases as cm
import flow_cases as fc
from test_gpu_rectify import pinned_schedule, same

pytestmark = pytest.mark.gpu

CASE_IDS = ["M"] + ["S-" + k for k in cc.S_KINDS]


@contextlib.contextmanager
def context(volib, w, h, max_pts=2048, max_frames=4, **params):
    ctx = volib.Context(0, w, h, max_pts, max_frames)
    try:
        if params:
            ctx.set_params(**params)
        pinned_schedule(ctx)
        yield ctx
    finally:
        ctx.close()


def the_case(name, small_seq, small_world):
    return cc.case_m(small_seq, small_world) if name == "M" else cc.case_s(name[2:], small_seq)


def same_bytes(a, b, what):
    assert all((x is None and y is None) or x.tobytes() == y.tobytes() for x, y in zip(a, b)), what


def sync_flow_calls(ctx, orc, prev, nxt, pair, pts, key, what):
    """the seven synchronous calls of the issue on (prev, nxt) as the context takes them, against the checker on `pair`"""
    want = cc.flow_want(orc, key, pair, pts)
    fc.assert_same(ctx.flow_track(prev, nxt, pts), want, (what, "voflow_track"))
    cc.assert_feature_tracking(ctx.feature_tracking(prev, nxt, pts), pts, want, (what, "voflow_feature_tracking"))
    for win in (5, 13):
        fc.assert_same(ctx.flow_track(prev, nxt, pts, win=win), cc.flow_want(orc, key, pair, pts, win=win), (what, "vowin_track", win))
    guess = cc.random_guess(pts)
    fc.assert_same(ctx.flow_track(prev, nxt, pts, guess=guess), cc.flow_want(orc, key, pair, pts, guess=guess), (what, "a guess"))
    n1, st, err = ctx.flow_track(prev, nxt, pts, min_eigenvals=True)
    fc.assert_same((n1, st, None), cc.flow_want(orc, key, pair, pts, min_eigenvals=True), (what, "min eigenvalues"))
    verified = cc.check_eig(orc, pair[0], pts, 21, err, (what, "min eigenvalues"))
    n1, st, err = ctx.flow_track(prev, nxt, pts, guess=guess, min_eigenvals=True)
    fc.assert_same((n1, st, None), cc.flow_want(orc, key, pair, pts, guess=guess, min_eigenvals=True), (what, "both flags"))
    assert cc.check_eig(orc, pair[0], pts, 21, err, (what, "both flags")) == verified
    return verified


# ---- 1. the synchronous flow calls with maps -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_IDS)
def test_sync_flow_calls_remap_both_images_through_the_left_maps(volib, orc, small_seq, small_world, name):
    c = the_case(name, small_seq, small_world)
    h, w = c["prev"].shape
    pair = cc.routed_pair(c)
    with context(volib, w, h, rectify=c["maps"]) as ctx:
        for set_name, pts in c["sets"].items():
            key = "%s-left-%s" % (c["tag"], set_name)
            verified = sync_flow_calls(ctx, orc, c["prev"], c["next"], pair, pts, key, (name, set_name))
            assert verified >= (590 if name == "M" else 50), verified
            assert ctx.flow_max_level(w, h) == cc.depth_of(c["prev"])
            # once more through a padded-stride view
            sync_flow_calls(ctx, orc, cc.padded(c["prev"]), cc.padded(c["next"]), pair, pts, key, (name, set_name, "padded"))


# ---- 2. the same with a format -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [cc.BGR8, cc.GRAY8_X2, cc.RGBA8], ids=lambda f: cc.NAMES[f])
def test_flow_calls_convert_then_remap(volib, orc, small_seq, small_world, fmt):
    c = cc.case_m(small_seq, small_world)
    a, b, pair = cc.colour_pair(c, fmt)
    key = "M-%s-left" % cc.NAMES[fmt]
    with context(volib, 480, 160, input_format=fmt, rectify=c["maps"]) as ctx:
        want = cc.flow_want(orc, key, pair, c["pts"])
        assert (want[1] == 1).sum() >= 450
        fc.assert_same(ctx.flow_track(a, b, c["pts"]), want, (cc.NAMES[fmt], "voflow_track"))
        cc.assert_feature_tracking(ctx.feature_tracking(a, b, c["pts"]), c["pts"], want, (cc.NAMES[fmt], "voflow_feature_tracking"))
        if fmt != cc.GRAY8_X2:   # (a plane of a two-byte interleave keeps its element stride: padded rows only)
            fc.assert_same(ctx.flow_track(cc.padded(a), cc.padded(b), c["pts"]), want, (cc.NAMES[fmt], "padded"))


@pytest.mark.parametrize("fmt", cc.FORMATS, ids=lambda f: cc.NAMES[f])
def test_flow_calls_convert_channels_that_differ(volib, orc, small_seq, small_world, fmt):
    """no maps: what the B = G = R image of the older tests cannot show -- channel order, weights, the byte plane"""
    c = cc.case_m(small_seq, small_world)
    a, b, pair = cc.colour_pair(c, fmt, "none")
    key = "M-%s-none" % cc.NAMES[fmt]
    pts = c["pts"]
    with context(volib, 480, 160, input_format=fmt) as ctx:
        want = cc.flow_want(orc, key, pair, pts)
        assert (want[1] == 1).sum() >= 450
        fc.assert_same(ctx.flow_track(a, b, pts), want, (cc.NAMES[fmt], "voflow_track"))
        fc.assert_same(ctx.flow_track(a, b, pts, win=13), cc.flow_want(orc, key, pair, pts, win=13), (cc.NAMES[fmt], "vowin_track", 13))
        guess = cc.random_guess(pts)
        fc.assert_same(ctx.flow_track(a, b, pts, guess=guess), cc.flow_want(orc, key, pair, pts, guess=guess), (cc.NAMES[fmt], "a guess"))


# ---- 3. what a flow call leaves behind ---------------------------------------------------------------------------------------------------
def test_a_flow_call_with_maps_leaves_a_context_fit_for_the_stereo_calls(volib, orc, small_seq, small_world):
    """slot 1 is rebuilt as it is and no stale flag stays set: the stereo calls that follow give a fresh context's bytes"""
    c = cc.case_m(small_seq, small_world)
    L, R, pts = small_seq["L"], small_seq["R"], small_seq["pts"][0]
    P_l, P_r = small_world.proj_matrices()
    pair = cc.routed_pair(c)
    with context(volib, 480, 160, rectify=c["maps"]) as ctx, context(volib, 480, 160, rectify=c["maps"]) as fresh:
        want4 = fresh.track_frame(L[0], R[0], L[1], R[1], pts, P_l, P_r)
        want4 = {k: np.array(v) for k, v in want4.items()}
        want_kept = fresh.track_frame(None, None, L[2], R[2], pts, P_l, P_r, tvec=want4["tvec"])
        want_kept = {k: np.array(v) for k, v in want_kept.items()}
        assert want4["rc"] == volib.VO_OK and len(want4["l1"]) >= 20 and want_kept["rc"] == volib.VO_OK and len(want_kept["l1"]) >= 20
        # the first call of the context (slot 1 was never written), then again behind a kept pair (every slot holds a pyramid)
        for turn, kw in enumerate((dict(), dict(win=13, guess=cc.random_guess(c["pts"])))):
            got = ctx.flow_track(c["prev"], c["next"], c["pts"], **kw)
            fc.assert_same(got, cc.flow_want(orc, "M-left-pts596", pair, c["pts"], win=kw.get("win", 21), guess=kw.get("guess")), ("turn", turn))
            assert ctx.kept_pair_id() == 0, "no kept pair after a flow call"
            with pytest.raises(volib.VoError) as e:
                ctx.track_frame(None, None, L[2], R[2], pts, P_l, P_r)
            assert e.value.code == volib.VO_ERR_STATE
            with pytest.raises(volib.VoError) as e:   # ... and no kept image for the detector either
                ctx.good_features_to_track(None, **cc.CORN)
            assert e.value.code == volib.VO_ERR_STATE
            got4 = ctx.track_frame(L[0], R[0], L[1], R[1], pts, P_l, P_r)
            same({k: np.array(v) for k, v in got4.items()}, want4, ("four images after a flow call, turn", turn))
            assert ctx.kept_pair_id() != 0
            got_kept = ctx.track_frame(None, None, L[2], R[2], pts, P_l, P_r, tvec=got4["tvec"])
            same({k: np.array(v) for k, v in got_kept.items()}, want_kept, ("the kept pair after a flow call, turn", turn))


# ---- 4. throughput mode --------------------------------------------------------------------------------------------------------------------
def upload_table(ctx, small_seq, n_frames):
    raw = cc.table_raw(small_seq)
    ctx.batch_configure(4, 480, 160, n_frames)
    for i, img in enumerate(raw):
        ctx.batch_upload_image(i, cc.padded(img) if i == 1 else img)
    return raw


def test_batch_flow_reads_a_table_rectified_by_parity(volib, orc, small_seq, small_world):
    pts = fc.point_sets(small_seq)["pts596"]
    rect = cc.table_rect(small_seq, small_world)
    pairs = cc.BATCH_PAIRS
    with context(volib, 480, 160, rectify=cc.m_maps(small_world)) as ctx:
        upload_table(ctx, small_seq, len(pairs))
        ctx.batch_run(volib.STAGE_PYRAMID)
        for f in range(len(pairs)):
            ctx.batch_set_points(f, pts)
        ctx.flow_batch_set_pairs(pairs)
        ctx.flow_batch_run()
        ctx.batch_sync()
        for f, (a, b) in enumerate(pairs):
            want = cc.flow_want(orc, "table-%d" % f, (rect[a], rect[b]), pts)
            assert (want[1] == 1).sum() >= 300
            fc.assert_same(ctx.flow_batch_get(f, len(pts)), want, ("voflow_batch_run, frame", f))
        ctx.flow_batch_run(win=13)
        for f, (a, b) in enumerate(pairs):
            fc.assert_same(ctx.flow_batch_get(f, len(pts)), cc.flow_want(orc, "table-%d" % f, (rect[a], rect[b]), pts, win=13), ("vowin_batch_run(13), frame", f))
        guesses = [cc.random_guess(pts, seed=20 + f) for f in range(len(pairs))]
        for f, g in enumerate(guesses):
            ctx.flow_batch_set_guess(f, g)
        ctx.flow_batch_run(guess=True)
        for f, (a, b) in enumerate(pairs):
            want = cc.flow_want(orc, "table-guess-%d" % f, (rect[a], rect[b]), pts, guess=guesses[f])
            fc.assert_same(ctx.flow_batch_get(f, len(pts)), want, ("voflag_batch_run with guesses, frame", f))


# ---- 5. corners ------------------------------------------------------------------------------------------------------------------------------
def test_corner_calls_with_maps(volib, orc, small_seq, small_world):
    """an image that is given: RAW (never rectified); img == NULL: the kept pair's left image, which was rectified; the table:
    rectified by parity; a mask: exactly as given, everywhere"""
    c = cc.case_m(small_seq, small_world)
    L, R, pts = small_seq["L"], small_seq["R"], small_seq["pts"][0]
    P_l, P_r = small_world.proj_matrices()
    raw, rect = c["next"], cc.routed_pair(c)[1]
    assert raw is L[1]
    masks = cc.corner_masks(480, 160)
    kept = cc.corn_want("M-L1-raw", raw)[:40] + np.float32(0.4)
    with context(volib, 480, 160, rectify=c["maps"]) as ctx:
        for view in (lambda a: a, cc.padded):
            cc.same_corners(ctx.good_features_to_track(view(raw), **cc.CORN), cc.corn_want("M-L1-raw", raw), "vocorn_detect reads the raw image")
            cc.same_map(ctx.corner_min_eigen_val(view(raw)), cc.map_want("M-L1-raw", raw), "vocorn_min_eigen_map reads the raw image")
        for name, m in masks.items():
            cc.same_corners(ctx.good_features_to_track(raw, mask=cc.padded(m, 9), **cc.CORN), cc.corn_want("M-L1-raw-" + name, raw, m),
                            ("vocmask_detect: raw image", name))
        disc = cm.ref_disc_mask(480, 160, kept, 5)
        cc.same_corners(ctx.replenish_corners(raw, kept, 5, max_corners=300), cc.corn_want("M-L1-raw-disc", raw, disc, 300), "vocmask_replenish: raw image")
        # the kept pair's left image went through the left maps
        r = ctx.track_frame(L[0], R[0], L[1], R[1], pts, P_l, P_r)
        assert r["rc"] == volib.VO_OK and ctx.kept_pair_id() != 0
        cc.same_corners(ctx.good_features_to_track(None, **cc.CORN), cc.corn_want("M-L1-left", rect), "vocorn_detect(NULL): the rectified left image")
        cc.same_map(ctx.corner_min_eigen_val(None), cc.map_want("M-L1-left", rect), "vocorn_min_eigen_map(NULL)")
        cc.same_corners(ctx.good_features_to_track(None, mask=masks["checker"], **cc.CORN), cc.corn_want("M-L1-left-checker", rect, masks["checker"]),
                        "vocmask_detect(NULL): the mask is not remapped")
        cc.same_corners(ctx.replenish_corners(None, kept, 5, max_corners=300), cc.corn_want("M-L1-left-disc", rect, disc, 300), "vocmask_replenish(NULL)")
        # an image of its own beside the kept pair leaves the pair in place, and is still the raw one
        cc.same_corners(ctx.good_features_to_track(raw, **cc.CORN), cc.corn_want("M-L1-raw", raw), "vocorn_detect beside a kept pair")
        cc.same_corners(ctx.good_features_to_track(None, **cc.CORN), cc.corn_want("M-L1-left", rect), "the kept image is still in place")
        # the table
        table = cc.table_rect(small_seq, small_world)
        upload_table(ctx, small_seq, 1)
        ctx.corners_batch_run(0, 4, **cc.CORN)
        for i in range(4):
            got, n = ctx.corners_batch_get(i)
            want = cc.corn_want("table-%d" % i, table[i])
            assert n == len(want) >= 500
            cc.same_corners(got, want, ("vocorn_batch_run, image", i))
        ctx.corners_batch_set_mask(2, cc.padded(masks["checker"], 3))
        ctx.corners_batch_set_mask(1, masks["left_half"])
        ctx.corners_batch_set_kept(3, kept, 6)
        ctx.corners_batch_run(0, 4, masked=True, **cc.CORN)
        expect = [cc.corn_want("table-0", table[0]), cc.corn_want("table-1-left_half", table[1], masks["left_half"]),
                  cc.corn_want("M-L1-left-checker", table[2], masks["checker"]),
                  cc.corn_want("table-3-disc", table[3], cm.ref_disc_mask(480, 160, kept, 6))]
        assert np.array_equal(table[2], rect)
        for i in range(4):
            got, n = ctx.corners_batch_get(i)
            assert n == len(expect[i]) >= 100
            cc.same_corners(got, expect[i], ("vocmask_batch_run, image", i))


def test_corner_calls_with_maps_and_a_colour_format(volib, small_seq, small_world):
    """the image is converted and not rectified, the mask is neither"""
    c = cc.case_m(small_seq, small_world)
    colour, gray, _ = cc.encode(c["next"], cc.BGR8, 62)
    mask = cc.corner_masks(480, 160)["checker"]
    with context(volib, 480, 160, input_format=cc.BGR8, rectify=c["maps"]) as ctx:
        want = cc.corn_want("M-L1-bgr8", gray)
        assert len(want) >= 500 and not np.array_equal(want[:50], cc.corn_want("M-L1-raw", c["next"])[:50])
        cc.same_corners(ctx.good_features_to_track(colour, **cc.CORN), want, "vocorn_detect, BGR8")
        cc.same_map(ctx.corner_min_eigen_val(cc.padded(colour)), cc.map_want("M-L1-bgr8", gray), "vocorn_min_eigen_map, BGR8")
        cc.same_corners(ctx.good_features_to_track(colour, mask=mask, **cc.CORN), cc.corn_want("M-L1-bgr8-checker", gray, mask), "vocmask_detect, BGR8")


# ---- 6. refusals, and the way back --------------------------------------------------------------------------------------------------------
def test_another_size_than_the_maps_is_refused_and_changes_nothing(volib, orc, small_seq, small_world):
    c = cc.case_m(small_seq, small_world)
    s = cc.case_s("all_ab", small_seq)
    pts = c["pts"]
    with context(volib, 480, 160, rectify=c["maps"]) as ctx:
        flow_before = ctx.flow_track(c["prev"], c["next"], pts)
        fc.assert_same(flow_before, cc.flow_want(orc, "M-left-pts596", cc.routed_pair(c), pts), "before")
        corn_before = ctx.good_features_to_track(c["next"], **cc.CORN)
        cc.same_corners(corn_before, cc.corn_want("M-L1-raw", c["next"]), "before")
        guess = cc.random_guess(s["pts"])
        refused = [lambda: ctx.flow_track(s["prev"], s["next"], s["pts"]),
                   lambda: ctx.feature_tracking(s["prev"], s["next"], s["pts"]),
                   lambda: ctx.flow_track(s["prev"], s["next"], s["pts"], win=13, guess=guess, min_eigenvals=True),
                   lambda: ctx.good_features_to_track(s["prev"], **cc.CORN),
                   lambda: ctx.corner_min_eigen_val(s["prev"]),
                   lambda: ctx.good_features_to_track(s["prev"], mask=cm.checker(96, 64), **cc.CORN),
                   lambda: ctx.replenish_corners(s["prev"], s["pts"][:5], 5)]
        for i, call in enumerate(refused):
            with pytest.raises(volib.VoError) as e:
                call()
            assert e.value.code == volib.VO_ERR_ARG and len(str(e.value)) > 10, (i, str(e.value))
            assert len(ctx.lib.vo_last_error(ctx.h)) > 10
        same_bytes(ctx.flow_track(c["prev"], c["next"], pts), flow_before, "voflow_track after the refusals")
        assert ctx.good_features_to_track(c["next"], **cc.CORN).tobytes() == corn_before.tobytes(), "vocorn_detect after the refusals"
        # without maps the context is a plain one: the raw pair, any size
        ctx.set_params(rectify=None)
        assert ctx.get_params().rectify == 0
        sync_flow_calls(ctx, orc, c["prev"], c["next"], (c["prev"], c["next"]), pts, "M-none-pts596", "maps off")
        fc.assert_same(ctx.flow_track(s["prev"], s["next"], s["pts"]), fc.case("crop", small_seq, orc)["want"], "maps off, 96 x 64")
        cc.same_corners(ctx.good_features_to_track(c["next"], **cc.CORN), cc.corn_want("M-L1-raw", c["next"]), "maps off: the raw image as before")
