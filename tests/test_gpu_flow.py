"""The two-image tracker of include/vo_flow.h on the MI355X: voflow_track, voflow_feature_tracking and the throughput mode against
the checker's calcOpticalFlowPyrLK (accum_mode 0) -- positions, status and err BIT FOR BIT, every point -- and against the python
restatement of deleteUnmatchFeatures (tests/flow_cases.py, which also asserts that no comparison is vacuous); that the calls
leave the rest of the context's behaviour alone; and an argument sweep of the five calls in a child process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import flow_cases as fc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def ctx(gpu_ctx):
    """the shared context with the default LK depth and gray input, before and after"""
    gpu_ctx.set_params(lk_max_level=3, input_format=0)
    yield gpu_ctx
    gpu_ctx.set_params(lk_max_level=3, input_format=0)


@pytest.mark.parametrize("name", list(fc.CASES))
def test_track_matches_checker(ctx, orc, small_seq, name):
    c = fc.case(name, small_seq, orc)
    fc.assert_not_vacuous(name, c)
    ctx.set_params(lk_max_level=c["max_level"])
    got = ctx.flow_track(c["prev"], c["next"], c["pts"])
    fc.assert_same(got, c["want"], name)


def test_track_variants_of_one_call(ctx, orc, small_seq, volib):
    """a padded-stride ROI view, a BGR image of the same gray values, err == NULL, n = 0 and n = 1: all the contiguous call"""
    c = fc.case("L0-L1", small_seq, orc)
    h, w = c["prev"].shape
    big = np.full((2, h + 9, w + 37), 200, np.uint8)
    big[0, 4:4 + h, 11:11 + w] = c["prev"]
    big[1, 4:4 + h, 11:11 + w] = c["next"]
    roi = ctx.flow_track(big[0, 4:4 + h, 11:11 + w], big[1, 4:4 + h, 11:11 + w], c["pts"])
    fc.assert_same(roi, c["want"], "ROI view")
    nxt, st, err = ctx.flow_track(c["prev"], c["next"], c["pts"], want_err=False)
    assert err is None
    fc.assert_same((nxt, st, None), c["want"], "err == NULL")
    nxt, st, err = ctx.flow_track(c["prev"], c["next"], c["pts"][:0])
    assert nxt.shape == (0, 2) and st.shape == (0,) and err.shape == (0,)
    one = ctx.flow_track(c["prev"], c["next"], c["pts"][:1])
    fc.assert_same(one, tuple(a[:1] for a in c["want"]), "n = 1")
    # cvtColor(BGR2GRAY) of a pixel with B = G = R = v is v: the colour call on the replicated image is the gray call
    ctx.set_params(input_format=volib.FMT_BGR8)
    bgr = ctx.flow_track(np.repeat(c["prev"][..., None], 3, 2), np.repeat(c["next"][..., None], 3, 2), c["pts"])
    ctx.set_params(input_format=volib.FMT_GRAY8)
    fc.assert_same(bgr, c["want"], "BGR8")


@pytest.mark.parametrize("name", ["L0-L1", "L0-R0"])
def test_feature_tracking_matches_delete_unmatch_features(ctx, orc, small_seq, name):
    c = fc.case(name, small_seq, orc)
    fc.assert_not_vacuous(name, c)
    nxt, st, err = c["want"]
    w0, w1, wst, wkeep = fc.delete_unmatch_features(c["pts"], nxt, st)
    assert 0 < len(wkeep) < (st == 1).sum() < len(st)
    r = ctx.feature_tracking(c["prev"], c["next"], c["pts"])
    assert r["n_out"] == len(wkeep) and np.array_equal(r["keep_idx"], wkeep) and np.array_equal(r["status"], wst)
    assert np.array_equal(fc.bits(r["points0"]), fc.bits(w0)) and np.array_equal(fc.bits(r["points1"]), fc.bits(w1))
    assert np.array_equal(fc.bits(r["err"]), fc.bits(err)), "err is not compacted"


def _batch(ctx, small_seq):
    L, R = small_seq["L"], small_seq["R"]
    imgs = [L[0], L[1], L[2], R[0], R[1]]
    pairs = [(0, 1), (1, 2), (0, 3), (3, 4), (2, 2), (1, 0)]
    counts = [596, 100, 0, 1, 64, 596]
    pts = np.ascontiguousarray(small_seq["pts"][0], np.float32)
    assert len(pts) == 596
    h, w = imgs[0].shape
    ctx.batch_configure(len(imgs), w, h, len(pairs))
    for i, im in enumerate(imgs):
        ctx.batch_upload_image(i, im)
    ctx.batch_run(1)   # VO_STAGE_PYRAMID
    for f, n in enumerate(counts):
        ctx.batch_set_points(f, pts[:n])
    ctx.flow_batch_set_pairs(pairs)
    return imgs, pairs, counts, pts


def test_batch_matches_checker_frame_by_frame(ctx, orc, small_seq):
    imgs, pairs, counts, pts = _batch(ctx, small_seq)
    ctx.flow_batch_run()
    ctx.batch_sync()
    first = [ctx.flow_batch_get(f, n) for f, n in enumerate(counts)]
    for f, ((a, b), n) in enumerate(zip(pairs, counts)):
        want = orc.calc_optical_flow_pyr_lk(imgs[a], imgs[b], pts[:n]) if n else (np.zeros((0, 2), np.float32), np.zeros(0, np.uint8), np.zeros(0, np.float32))
        fc.assert_same(first[f], want, "frame %d" % f)
    assert (first[0][1] == 0).sum() >= 20 and (first[0][1] == 1).sum() >= 500 and (first[5][2] > 0).sum() >= 500
    ctx.flow_batch_run()
    again = [ctx.flow_batch_get(f, n) for f, n in enumerate(counts)]
    for a, b in zip(first, again):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), "a second voflow_batch_run gives identical bytes"


def _same_results(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)


def test_flow_calls_leave_the_stereo_calls_alone(ctx, orc, small_seq, small_world, volib):
    L, R, pts = small_seq["L"], small_seq["R"], small_seq["pts"][0]
    P_l, P_r = small_world.proj_matrices()
    before = ctx.track_frame(L[0], R[0], L[1], R[1], pts, P_l, P_r)
    before = {k: np.array(v) for k, v in before.items()}
    assert ctx.kept_pair_id() != 0
    c = fc.case("crop", small_seq, orc)
    ctx.flow_track(c["prev"], c["next"], c["pts"])
    assert ctx.kept_pair_id() == 0, "no kept pair after voflow_track"
    with pytest.raises(volib.VoError) as e:
        ctx.track_frame(None, None, L[1], R[1], pts, P_l, P_r)
    assert e.value.code == volib.VO_ERR_STATE
    ctx.feature_tracking(L[0], L[1], pts)
    ctx.flow_track(L[1], L[2], pts[:50], want_err=False)
    _batch(ctx, small_seq)
    ctx.flow_batch_run()
    ctx.batch_sync()
    after = ctx.track_frame(L[0], R[0], L[1], R[1], pts, P_l, P_r)
    assert _same_results(before, after), "vo_track_frame before and after a series of flow calls"


def test_batch_run_after_flow_batch_run_equals_a_fresh_context(ctx, small_seq, small_world, volib):
    L, R, pts = small_seq["L"], small_seq["R"], small_seq["pts"][0]
    P_l, P_r = small_world.proj_matrices()
    h, w = L[0].shape

    def stereo_batch(cx, flow):
        cx.batch_configure(4, w, h, 1)
        for i, im in enumerate((L[0], R[0], L[1], R[1])):
            cx.batch_upload_image(i, im)
        cx.batch_set_projection(P_l, P_r)
        cx.batch_set_points(0, pts)
        if flow:
            cx.batch_run(1)
            cx.flow_batch_set_pairs([(0, 2)])
            cx.flow_batch_run()
        cx.batch_set_quads([(0, 1, 2, 3)])
        cx.batch_run()
        cx.batch_sync()
        return dict(cx.batch_get_filtered(0), **{"pose_" + k: np.asarray(v) for k, v in cx.batch_get_pose(0).items()})

    got = stereo_batch(ctx, True)
    fresh = volib.Context(0, 640, 480, 1024, 1)
    try:
        want = stereo_batch(fresh, False)
    finally:
        fresh.close()
    assert len(got["l0"]) > 100 and _same_results(want, got)


def test_argument_sweep_of_the_flow_calls():
    """tests/flow_sweep.py in a child process (a fault must fail THIS test, not end the session)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "flow_sweep.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode in (0, 1), "flow_sweep died (rc %d): %s" % (r.returncode, r.stderr[-2000:])
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    assert not rep["failures"], rep["failures"]
    assert rep["checked"] >= 40
    from visual_odom_amd import _lib
    assert sorted(rep["covered"]) == sorted(_lib.FLOW_EXPORTS)
