"""The cases of tests/test_lk_tile_emulation.py on the MI355X, through the C ABI: the 4-hop chain in batches of 1, 3 and 9 frames
at 131 x 97 and 169 x 169 against the checker, the kept-pair call (lk_hops_kernel [0, 1) + [1, 4)) against the four-image call,
and the two-image calls of four windows with err and with each flag.  Everything bit for bit."""
import numpy as np
import pytest

import flow_cases as fc
import flow_flags_cases as gc
import lk_chain_cases as lc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(volib):
    c = volib.Context(0, 256, 256, 512, 9)
    yield c
    c.close()


@pytest.mark.parametrize("n_frames", lc.BATCHES)
@pytest.mark.parametrize("shape", lc.SHAPES, ids=lambda s: "%dx%d" % s)
def test_chain_in_batches(ctx, volib, orc, shape, n_frames):
    lc.chain_premises(shape, lc.oracle_chain(orc, shape, 0))
    w, h = shape
    pts, n = lc.points(shape), len(lc.points(shape))
    cnt = lc.counts(n_frames, n)
    ctx.set_params(lk_full_chain=1, lk_max_level=3)
    try:
        ctx.batch_configure(4, w, h, n_frames)
        for i, im in enumerate(lc.images(shape)):
            ctx.batch_upload_image(i, im)
        ctx.batch_set_quads(lc.quads(n_frames))
        for f in range(n_frames):
            ctx.batch_set_points(f, pts[:cnt[f]])
        ctx.batch_run(volib.STAGE_PYRAMID | volib.STAGE_LK)
        ctx.batch_sync()
        trk, st = np.zeros((n_frames, 4, n, 2), np.float32), np.zeros((n_frames, 4, n), np.uint8)
        for f in range(n_frames):
            g = ctx.batch_get_tracks(f, int(cnt[f]))
            st[f][:, :cnt[f]] = g["status4"]
            for hop, name in enumerate(("r0", "r1", "l1", "l0_ret")):
                trk[f][hop, :cnt[f]] = g[name]
    finally:
        ctx.set_params(lk_full_chain=0)
    lc.assert_chain(orc, shape, (trk, st, cnt), "batch of %d" % n_frames)


@pytest.mark.parametrize("shape", lc.SHAPES, ids=lambda s: "%dx%d" % s)
def test_kept_pair_call_equals_four_image_call(volib, shape):
    """vo_circular_match on the kept pair launches hop 0, then hops 1 .. 3 (capi_run.hip); a second context gets all four images"""
    w, h = shape
    im, pts = lc.images(shape), lc.points(shape)
    a, b = volib.Context(0, w, h, 512, 1), volib.Context(0, w, h, 512, 1)
    try:
        a.circular_match(im[2], im[3], im[0], im[1], pts)          # leaves the pair (0, 1)
        got = a.circular_match(None, None, im[2], im[3], pts)
        want = b.circular_match(im[0], im[1], im[2], im[3], pts)
        assert (want["status4"] == 0).any() and want["n_out"] >= 10
        for key in ("l0", "r0", "r1", "l1", "l0_ret", "status4", "keep_idx"):
            assert np.array_equal(got[key], want[key], equal_nan=True), key
    finally:
        a.close()
        b.close()


def _track(ctx, c, **kw):
    ctx.set_params(lk_max_level=c["lk_max_level"])
    return ctx.flow_track(c["prev"], c["next"], c["pts"], win=None if c["win"] == 21 and not kw else c["win"], **kw)


@pytest.mark.parametrize("win", lc.WINDOWS)
@pytest.mark.parametrize("shape", lc.SHAPES, ids=lambda s: "%dx%d" % s)
def test_two_image_calls(ctx, orc, shape, win):
    """err (voflow_track at 21, vowin_track below), USE_INITIAL_FLOW and GET_MIN_EIGENVALS (voflag_track) of one window"""
    try:
        c = lc.flow_case(shape, win, orc)
        assert ctx.flow_max_level(*shape) == c["max_level"]
        assert (c["want"][1] == 1).sum() >= 15 and (c["want"][1] == 0).sum() >= 15 and (c["want"][2] > 0).any()
        fc.assert_same(_track(ctx, c), c["want"], (shape, win, "err"))
        g = lc.guess_case(shape, win, orc)
        fc.assert_same(_track(ctx, g, guess=g["guess"]), g["want"], (shape, win, "guess"))
        s = lc.eig_set(shape, win, orc)
        e = dict(prev=s["img"], next=s["img"], pts=s["pts"], win=win, lk_max_level=0)
        gc.check_min_eigenvals(orc, s, _track(ctx, e, min_eigenvals=True), (shape, win, "min eigenvalue"))
    finally:
        ctx.set_params(lk_max_level=3)


@pytest.mark.parametrize("win", lc.ALL_WINDOWS)
def test_flag_kernels_of_every_window(ctx, orc, win):
    """lk_flow_flags_kernel<W> is nine binaries: voflag_track of each with a guess and with min_eigenvals against the checker
    (tests/test_lk_tile_emulation.py runs the same cases on the emulator)"""
    shape = lc.SHAPES[0]
    try:
        g, s, e = lc.flag_cases(shape, win, orc)
        fc.assert_same(_track(ctx, g, guess=g["guess"]), g["want"], (shape, win, "guess"))
        gc.check_min_eigenvals(orc, s, _track(ctx, e, min_eigenvals=True), (shape, win, "min eigenvalue"))
    finally:
        ctx.set_params(lk_max_level=3)
