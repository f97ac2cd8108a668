"""The LK iteration with one loop per kind of sum and a scalar branch on iw11 = -1, on the MI355X: the 160 x 120 cases of
tests/lk_branches.py (the three images of tests/lk_fit.py -- every level's sums fit 32 bits, none does, both -- and one image four
times; 64 points, eight of which start at a window corner whose weights have iw11 = -1) through vo_batch_* with 8 frames
(lk_circular_kernel) and 16 frames (lk_circular_queue_kernel), every frame against the checker's chain bit for bit, and through the
two-image call with windows 21 and 5.  Which loop and which blend a case runs is shown on the CPU emulator
(tests/test_lk_iteration_branches_emulation.py), which runs the same source."""
import numpy as np
import pytest

import flow_cases as fc
import lk_branches
import lk_fit

pytestmark = pytest.mark.gpu
KINDS = ("low", "checker", "synth", "still")


@pytest.fixture(scope="module")
def ctx(volib):
    c = volib.Context(0, lk_fit.W, lk_fit.H, lk_fit.N_PTS, 16)
    c.set_params(lk_full_chain=1, lk_max_level=3, lk_max_count=30, lk_min_eig_threshold=0.001)
    yield c
    c.close()


@pytest.mark.parametrize("n_frames", [8, 16], ids=["8-static", "16-queue"])
@pytest.mark.parametrize("kind", KINDS)
def test_batch_chain_matches_checker(ctx, volib, orc, kind, n_frames):
    want_trk, want_st = lk_branches.oracle_chain(orc, kind)
    assert (want_st[3] == 1).sum() >= 32
    pts = lk_branches.points()
    ctx.batch_configure(4, lk_fit.W, lk_fit.H, n_frames)
    for i, im in enumerate(lk_branches.images(kind)):
        ctx.batch_upload_image(i, im)
    ctx.batch_set_quads(np.ascontiguousarray(np.tile(np.arange(4, dtype=np.int32), (n_frames, 1))))
    for f in range(n_frames):
        ctx.batch_set_points(f, pts)
    ctx.batch_run(volib.STAGE_PYRAMID | volib.STAGE_LK)
    ctx.batch_sync()
    for f in range(n_frames):
        g = ctx.batch_get_tracks(f, len(pts))
        trk = np.stack([g[key] for key in ("r0", "r1", "l1", "l0_ret")])
        assert np.array_equal(g["status4"], want_st), (kind, n_frames, f, "status")
        assert np.array_equal(fc.bits(trk), fc.bits(want_trk)), (kind, n_frames, f, "positions")


@pytest.mark.parametrize("win", [21, 5])
@pytest.mark.parametrize("kind", KINDS)
def test_flow_call_matches_checker(gpu_ctx, orc, kind, win):
    c = lk_branches.flow_case(orc, kind, win)
    gpu_ctx.set_params(lk_max_level=3, input_format=0)
    assert gpu_ctx.flow_max_level(lk_fit.W, lk_fit.H) == c["max_level"]
    fc.assert_same(gpu_ctx.flow_track(c["prev"], c["next"], c["pts"], win=win), c["want"], (kind, win))
