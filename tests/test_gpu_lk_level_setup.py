"""The cases of tests/test_lk_level_setup.py on the MI355X: every case a frame of one batch through the C ABI (lk_circular_kernel),
one launch per parameter set; the negative-coordinate case through the kept-pair call (lk_hops_kernel [0, 1) + [1, 4)); one case
through the two-image calls at windows 5, 13 and 21 with err; and the reciprocal of the determinant (vo_isa.h, rcp_normal_f32)
against the device's IEEE division on every float of its range.  Status on every hop, positions as raw bits on every hop the
checker reports alive, err bit for bit where the checker's status is 1."""
import numpy as np
import pytest

import lk_rcp
import lk_setup_cases as sc

pytestmark = pytest.mark.gpu

SMALL = tuple(n for n in sc.CASES if n != "deep")


@pytest.fixture(scope="module")
def ctx(volib):
    c = volib.Context(0, sc.W, sc.H_DEEP, 64, len(SMALL))
    yield c
    c.close()


def _defaults(ctx):
    ctx.set_params(lk_full_chain=0, lk_max_level=3, lk_max_count=30, lk_min_eig_threshold=0.001)


def test_the_cases_take_their_paths(orc):
    sc.premises(orc)


@pytest.mark.parametrize("prm", sc.PARAMS, ids=lambda p: "L%d-n%d-e%g" % p)
@pytest.mark.parametrize("names", [SMALL, ("deep",)], ids=["96x64", "96x88"])
def test_batch_chain_equals_checker(ctx, volib, orc, names, prm):
    cases = [sc.case(name) for name in names]
    nf, h = len(cases), cases[0]["h"]
    ctx.set_params(lk_full_chain=1, lk_max_level=prm[0], lk_max_count=prm[1], lk_min_eig_threshold=prm[2])
    try:
        ctx.batch_configure(4 * nf, sc.W, h, nf)
        for f, c in enumerate(cases):
            for i, im in enumerate(c["imgs"]):
                ctx.batch_upload_image(4 * f + i, im)
        ctx.batch_set_quads(np.arange(4 * nf, dtype=np.int32).reshape(nf, 4))
        for f, c in enumerate(cases):
            ctx.batch_set_points(f, c["pts"])
        ctx.batch_run(volib.STAGE_PYRAMID | volib.STAGE_LK)
        ctx.batch_sync()
        for f, (name, c) in enumerate(zip(names, cases)):
            g = ctx.batch_get_tracks(f, len(c["pts"]))
            trk = np.stack([g[k] for k in ("r0", "r1", "l1", "l0_ret")])
            sc.assert_chain(trk, g["status4"], sc.oracle(orc, name, prm), (name, prm))
    finally:
        _defaults(ctx)


def test_kept_pair_call_equals_checker(volib, orc):
    """vo_circular_match on the kept pair launches hop 0, then hops 1 .. 3 (lk_hops_kernel): the points outside the image"""
    name, prm = "outside", sc.PARAMS[1]
    c, want = sc.case("outside"), sc.oracle(orc, "outside", sc.PARAMS[1])
    im, pts = c["imgs"], c["pts"]
    a = volib.Context(0, sc.W, sc.H, 64, 1)
    try:
        a.set_params(lk_full_chain=1, lk_max_level=prm[0], lk_max_count=prm[1], lk_min_eig_threshold=prm[2])
        a.circular_match(im[2], im[3], im[0], im[1], pts)          # leaves the pair (0, 1)
        got = a.circular_match(None, None, im[2], im[3], pts)
    finally:
        a.close()
    assert np.array_equal(got["status4"], want["status"]), name
    # the survivors of deleteUnmatchFeaturesCircle: every hop alive, no negative coordinate
    keep = got["keep_idx"]
    assert len(keep) >= 5 and (want["status"][:, keep] == 1).all()
    for hop, key in enumerate(("r0", "r1", "l1", "l0_ret")):
        assert np.array_equal(sc.bits(got[key]), sc.bits(want["trk"][hop][keep])), key


@pytest.mark.parametrize("win", [5, 13, 21])
def test_two_image_call_equals_checker(ctx, orc, win):
    """voflow_track (21) / vowin_track (5, 13): the body with the err epilogue, on the points outside the image and on the jump"""
    try:
        for name in ("outside", "jump"):
            c, lost = sc.case(name), 0
            for prm in (sc.PARAMS[1], sc.PARAMS[4], sc.PARAMS[6]):
                ctx.set_params(lk_max_level=prm[0], lk_max_count=prm[1], lk_min_eig_threshold=prm[2])
                nxt, st, err = ctx.flow_track(c["imgs"][0], c["imgs"][1], c["pts"], win=None if win == 21 else win)
                # (the library's pyramid stops where a level would not be larger than 21, whatever the window: the checker is asked
                # for that depth, as include/vo_flow_win.h says)
                depth = ctx.flow_max_level(sc.W, sc.H)
                assert depth == sc.depth(sc.H, prm[0])
                wn, ws, we = sc.oracle_flow(orc, name, (depth, prm[1], prm[2]), win)
                assert np.array_equal(st, ws), (name, prm, "status")
                alive = ws == 1
                assert alive.any()
                lost += int((~alive).sum())
                assert (sc.bits(nxt) == sc.bits(wn)).all(-1)[alive].all(), (name, prm, "positions")
                assert np.array_equal(sc.bits(err)[alive], sc.bits(we)[alive]), (name, prm, "err")
            assert lost > 0, (name, "no point of the sweep was refused")   # (lk_max_count = 0 on "jump" refuses none: no iteration)
    finally:
        _defaults(ctx)


def test_reciprocal_of_the_determinant_on_the_device(tmp_path):
    """rcp_normal_f32 against the device's 1.0f / x on all 52 * 2^23 floats of [2^-23, 2^29): no mismatch; and the device's
    quotients of 2^20 evenly spaced operands byte for byte a g++ build's.  One start of each program."""
    d = str(tmp_path)
    host, dev = lk_rcp.build_host(d), lk_rcp.build_device(d)
    assert lk_rcp.run(host, str(tmp_path / "host.out")) == [lk_rcp.SAMPLES]
    assert lk_rcp.run(dev, str(tmp_path / "dev.out")) == [lk_rcp.OPERANDS, 0]    # a mismatch is exit 1: it failed in run()
    want = np.fromfile(str(tmp_path / "host.out"), np.uint32)
    got = np.fromfile(str(tmp_path / "dev.out"), np.uint32)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, ("device 1.0f / x != g++ build", len(bad), int(bad[0]), hex(got[bad[0]]), hex(want[bad[0]]))
