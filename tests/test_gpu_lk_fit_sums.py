"""The 32-bit iteration sums on the MI355X.
  * The vectors of tests/host_check/lk_fit_cases.h through wave_sum2_fit_f32, wave_sum2_exact_f32 and wave_sum2_f32 on gfx950
    (lk_fit_check.hip: one small program, built with the product's flags, started ONCE); the records it wrote equal, byte for byte,
    those of the g++ program over the emulator text (lk_fit_host.cpp).
  * The three 160 x 120 cases of tests/lk_fit.py (every level fits / none does / both) through vo_batch_*: 8 frames (lk_circular_kernel)
    and 16 frames (lk_circular_queue_kernel), every frame against the checker's chain bit for bit; and through the two-image call
    with windows 21 and 5.  Which sums a case runs with is shown on the CPU emulator (tests/test_lk_fit_sums_emulation.py)."""
import numpy as np
import pytest

import flow_cases as fc
import lk_fit

pytestmark = pytest.mark.gpu
KINDS = ("low", "checker", "synth")


def test_fit_sums_on_the_device(tmp_path):
    d = str(tmp_path)
    host, dev = lk_fit.build_host(d), lk_fit.build_device(d)
    n_host = lk_fit.run(host, str(tmp_path / "host.out"))
    n_dev = lk_fit.run(dev, str(tmp_path / "dev.out"))       # a non-zero exit, a signal or the time limit fails here: no second run
    assert n_dev == n_host[:2] and n_dev[0] >= 1000 and n_dev[1] >= 400
    want = np.fromfile(str(tmp_path / "host.out"), np.uint32).reshape(-1, 6)
    got = np.fromfile(str(tmp_path / "dev.out"), np.uint32).reshape(-1, 6)
    bad = np.flatnonzero((got != want).any(1))
    assert len(bad) == 0, ("device != emulator text", len(bad), int(bad[0]), got[bad[0]], want[bad[0]])


@pytest.fixture(scope="module")
def ctx(volib):
    c = volib.Context(0, lk_fit.W, lk_fit.H, lk_fit.N_PTS, 16)
    c.set_params(lk_full_chain=1, lk_max_level=3, lk_max_count=30, lk_min_eig_threshold=0.001)
    yield c
    c.close()


@pytest.mark.parametrize("n_frames", [8, 16], ids=["8-static", "16-queue"])
@pytest.mark.parametrize("kind", KINDS)
def test_batch_chain_matches_checker(ctx, volib, orc, kind, n_frames):
    want_trk, want_st = lk_fit.oracle_chain(orc, kind)
    assert (want_st[3] == 1).sum() >= 32
    pts = lk_fit.points()
    ctx.batch_configure(4, lk_fit.W, lk_fit.H, n_frames)
    for i, im in enumerate(lk_fit.images(kind)):
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
    c = lk_fit.flow_case(orc, kind, win)
    gpu_ctx.set_params(lk_max_level=3, input_format=0)
    assert gpu_ctx.flow_max_level(lk_fit.W, lk_fit.H) == c["max_level"]
    fc.assert_same(gpu_ctx.flow_track(c["prev"], c["next"], c["pts"], win=win), c["want"], (kind, win))
