"""The windowed two-image tracker of include/vo_flow_win.h on the MI355X: vowin_track, vowin_feature_tracking, vowin_batch_run and
vowin_max_level.  The expected side of every comparison is the checker's calcOpticalFlowPyrLK(win=W, max_level=E) (accum_mode 0),
E being the depth the library plans (tests/flow_win_cases.py: the cases, the rule, and the premises asserted first) -- positions,
status and err BIT FOR BIT, every point.  Also: window 21 is the voflow_* call, the calls leave the rest of the context alone, and
an argument sweep in a child process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import flow_cases as fc
import flow_win_cases as wc
from test_gpu_flow import _batch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def ctx(gpu_ctx):
    """the shared context with the default LK depth and gray input, before and after"""
    gpu_ctx.set_params(lk_max_level=3, input_format=0)
    yield gpu_ctx
    gpu_ctx.set_params(lk_max_level=3, input_format=0)


@pytest.mark.parametrize("name", ["crop", "lattice", "L0-L1"])
@pytest.mark.parametrize("win", wc.WINDOWS)
def test_track_matches_checker(ctx, orc, small_seq, win, name):
    c = wc.case(name, win, small_seq, orc)
    wc.premises(name, c)
    if name == "L0-L1":   # what makes a wrong depth or an ignored window fail this comparison
        assert wc.depth_premise(win, small_seq, orc) >= 500 and wc.window_premise(win, small_seq, orc) >= 590
    ctx.set_params(lk_max_level=c["lk_max_level"])
    h, w = c["prev"].shape
    assert ctx.flow_max_level(w, h) == c["max_level"]
    fc.assert_same(ctx.flow_track(c["prev"], c["next"], c["pts"], win=win), c["want"], (name, win))


def test_kitti_size_is_opencvs_own_call(ctx, orc, kitti_seq):
    """1241 x 376: every level down to lk_max_level is larger than 21, E = 3 = maxLevel of the plain OpenCV call"""
    L, pts = kitti_seq["L"], np.ascontiguousarray(kitti_seq["pts"][:400], np.float32)
    assert len(pts) == 400 and ctx.flow_max_level(1241, 376) == 3
    want = orc.calc_optical_flow_pyr_lk(L[0], L[1], pts, win=15, max_level=3)
    assert (want[1] == 1).sum() >= 200 and np.all(want[2][want[1] == 1] > 0)
    fc.assert_same(ctx.flow_track(L[0], L[1], pts, win=15), want, "kitti 15")


def test_max_level_follows_the_rule(ctx):
    want = {(1241, 376): [0, 1, 2, 3, 4], (480, 160): [0, 1, 2, 2, 2], (96, 64): [0, 1, 1, 1, 1]}
    for (w, h), levels in want.items():
        for ml in range(5):
            ctx.set_params(lk_max_level=ml)
            assert ctx.flow_max_level(w, h) == levels[ml] == wc.depth(w, h, ml), (w, h, ml)


@pytest.mark.parametrize("win", [7, 15])
def test_feature_tracking_matches_delete_unmatch_features(ctx, orc, small_seq, win):
    c = wc.case("L0-R0", win, small_seq, orc)
    wc.premises("L0-R0", c)
    nxt, st, err = c["want"]
    w0, w1, wst, wkeep = fc.delete_unmatch_features(c["pts"], nxt, st)
    assert 0 < len(wkeep) < (st == 1).sum() < len(st)
    r = ctx.feature_tracking(c["prev"], c["next"], c["pts"], win=win)
    assert r["n_out"] == len(wkeep) and np.array_equal(r["keep_idx"], wkeep) and np.array_equal(r["status"], wst)
    assert np.array_equal(fc.bits(r["points0"]), fc.bits(w0)) and np.array_equal(fc.bits(r["points1"]), fc.bits(w1))
    assert np.array_equal(fc.bits(r["err"]), fc.bits(err)), "err is not compacted"


def test_batch_matches_checker_frame_by_frame(ctx, orc, small_seq):
    imgs, pairs, counts, pts = _batch(ctx, small_seq)
    empty = (np.zeros((0, 2), np.float32), np.zeros(0, np.uint8), np.zeros(0, np.float32))
    for win in (7, 15):
        ctx.flow_batch_run(win=win)
        got = [ctx.flow_batch_get(f, n) for f, n in enumerate(counts)]
        for f, ((a, b), n) in enumerate(zip(pairs, counts)):
            want = orc.calc_optical_flow_pyr_lk(imgs[a], imgs[b], pts[:n], win=win, max_level=2) if n else empty
            fc.assert_same(got[f], want, "win %d frame %d" % (win, f))
        assert (got[0][1] == 0).sum() >= 30 and (got[0][1] == 1).sum() >= 500 and (got[5][2] > 0).sum() >= 500
    ctx.flow_batch_run()
    plain = [ctx.flow_batch_get(f, n) for f, n in enumerate(counts)]
    ctx.flow_batch_run(win=7)   # (something else in the result buffers in between)
    ctx.flow_batch_run(win=21)
    w21 = [ctx.flow_batch_get(f, n) for f, n in enumerate(counts)]
    for a, b in zip(plain, w21):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), "vowin_batch_run(21) gives the bytes of voflow_batch_run"


def test_window_21_is_voflow_track(ctx, orc, small_seq):
    c = fc.case("L0-L1", small_seq, orc)
    plain = ctx.flow_track(c["prev"], c["next"], c["pts"])
    w21 = ctx.flow_track(c["prev"], c["next"], c["pts"], win=21)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(plain, w21))
    fc.assert_same(w21, c["want"], "win 21")


def test_track_variants_of_one_call(ctx, orc, small_seq, volib):
    """a padded-stride ROI view and a BGR image of the same gray values are the contiguous gray call, at W = 9"""
    c = wc.case("L0-L1", 9, small_seq, orc)
    h, w = c["prev"].shape
    big = np.full((2, h + 9, w + 37), 200, np.uint8)
    big[0, 4:4 + h, 11:11 + w] = c["prev"]
    big[1, 4:4 + h, 11:11 + w] = c["next"]
    fc.assert_same(ctx.flow_track(big[0, 4:4 + h, 11:11 + w], big[1, 4:4 + h, 11:11 + w], c["pts"], win=9), c["want"], "ROI view")
    nxt, st, err = ctx.flow_track(c["prev"], c["next"], c["pts"], want_err=False, win=9)
    assert err is None
    fc.assert_same((nxt, st, None), c["want"], "err == NULL")
    ctx.set_params(input_format=volib.FMT_BGR8)
    bgr = ctx.flow_track(np.repeat(c["prev"][..., None], 3, 2), np.repeat(c["next"][..., None], 3, 2), c["pts"], win=9)
    ctx.set_params(input_format=volib.FMT_GRAY8)
    fc.assert_same(bgr, c["want"], "BGR8")


def test_windowed_calls_leave_the_other_calls_alone(ctx, orc, small_seq):
    L, R, pts = small_seq["L"], small_seq["R"], small_seq["pts"][0]
    c = fc.case("L0-L1", small_seq, orc)
    flow_before = ctx.flow_track(c["prev"], c["next"], c["pts"])
    circ_before = {k: np.array(v) for k, v in ctx.circular_match(L[0], R[0], L[1], R[1], pts).items()}
    assert circ_before["n_out"] > 100
    for win in (5, 13, 19):
        ctx.flow_track(c["prev"], c["next"], c["pts"], win=win)
    ctx.feature_tracking(L[0], R[0], pts, win=9)
    assert ctx.kept_pair_id() == 0, "no kept pair after a windowed call"
    _batch(ctx, small_seq)
    ctx.flow_batch_run(win=11)
    ctx.batch_sync()
    flow_after = ctx.flow_track(c["prev"], c["next"], c["pts"])
    circ_after = ctx.circular_match(L[0], R[0], L[1], R[1], pts)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(flow_before, flow_after))
    assert all(np.asarray(circ_before[k]).tobytes() == np.asarray(circ_after[k]).tobytes() for k in circ_before)
    fc.assert_same(flow_after, c["want"], "voflow_track after windowed calls")


def test_argument_sweep_of_the_win_calls():
    """tests/flow_win_sweep.py in a child process (a fault must fail THIS test, not end the session)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "flow_win_sweep.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode in (0, 1), "flow_win_sweep died (rc %d): %s" % (r.returncode, r.stderr[-2000:])
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    assert not rep["failures"], rep["failures"]
    assert rep["checked"] >= 60
    from visual_odom_amd import _lib
    assert sorted(rep["covered"]) == sorted(_lib.WIN_EXPORTS)
