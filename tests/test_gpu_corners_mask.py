"""The Shi-Tomasi detector under a mask (include/vo_corners_mask.h) on the device, held BIT FOR BIT -- corner lists with their order,
and the disc mask byte for byte; identity, no tolerance -- to the reference of corners_mask_cases.py, over the case table of the
emulator tests at the sizes a context takes: vocmask_detect, vocmask_disc_mask, vocmask_replenish, vocmask_batch_* and the errors."""
import ctypes as C

import numpy as np
import pytest

import corners_emu as ce
import corners_mask_cases as cm

pytestmark = pytest.mark.gpu

SHAPES = [(32, 32), (33, 35), (65, 33), (131, 67), (300, 40)]


@pytest.fixture(scope="module")
def ctx(volib):
    c = volib.Context(0, 320, 128, 256, 4)
    yield c
    c.close()


def padded(a, extra=5):
    """the array as a view of a wider one: a byte stride that is not the width"""
    h, w = a.shape
    buf = np.full((h, w + extra), 0xEE, np.uint8)
    buf[:, :w] = a
    return buf[:, :w]


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_detect_and_replenish_bit_for_bit(ctx, shape):
    w, h = shape
    for name, img, mask, mc, q, md in cm.mask_cases(w, h):
        want, n, _ = cm.ref_detect(img, mask, mc, q, md)
        got = ctx.good_features_to_track(padded(img), mc, q, md, mask=padded(mask, 9))
        assert len(got) == n and np.array_equal(got, want), name
        if name == "strong_outside" and shape in cm.STRONG_OUTSIDE_CORNERS:
            assert n == cm.STRONG_OUTSIDE_CORNERS[shape]
        if "all_zero" in name or "border_ring" in name:
            assert n == 0
        if "all_255" in name or "all_1" in name:
            assert np.array_equal(got, ctx.good_features_to_track(padded(img), mc, q, md)), name   # the bytes of vocorn_detect
    img = ce.noise(w, h, 23)
    kept = ce.ref_detect(img, 12, 0.01, 8.0)[0] + np.float32(0.4)
    for r, mc in ((5, 0), (1, 9), (0, 0)):
        want, n, _ = cm.ref_detect(img, cm.ref_disc_mask(w, h, kept, r), mc, 0.01, 5.0)
        got = ctx.replenish_corners(padded(img), kept, r, mc, 0.01, 5.0)
        assert len(got) == n and np.array_equal(got, want), (r, mc)
    # no kept point: the unmasked call; a radius that covers the image: nothing
    assert np.array_equal(ctx.replenish_corners(img, np.zeros((0, 2)), 5, 0, 0.01, 5.0), ce.ref_detect(img, 0, 0.01, 5.0)[0])
    assert len(ctx.replenish_corners(img, [(w / 2, h / 2)], 256, 0, 0.01, 5.0)) == 0
    # mask == NULL is vocorn_detect
    pts = np.zeros((w * h, 2), np.float32)
    cnt = C.c_int(0)
    assert ctx.lib.vocmask_detect(ctx.h, img.ctypes.data, w, h, w, None, 0, None, pts.ctypes.data, w * h, C.byref(cnt)) == 0
    want, n, _ = ce.ref_detect(img, 5000, 0.01, 5.0)   # (NULL params: the defaults)
    assert cnt.value == n and np.array_equal(pts[:n], want)


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_disc_mask_is_the_definition(ctx, volib, shape):
    w, h = shape
    for name, kept, r in cm.disc_cases(w, h):
        assert np.array_equal(ctx.corner_disc_mask(w, h, kept, r), cm.ref_disc_mask(w, h, kept, r)), name
    # a strided output: the bytes between the rows are left alone
    kept = np.array([(3.5, 4.5), (w - 1.0, h - 1.0)], np.float32)
    out = np.full((h, w + 7), 0x5A, np.uint8)
    assert ctx.lib.vocmask_disc_mask(ctx.h, w, h, kept.ctypes.data, 2, 3, out.ctypes.data, w + 7) == 0
    assert np.array_equal(out[:, :w], cm.ref_disc_mask(w, h, kept, 3)) and (out[:, w:] == 0x5A).all()


def test_batch_masks_ranges_and_configure_drops_them(ctx):
    w, h = 131, 67
    imgs = [ce.noise(w, h, 7), ce.blobs(w, h, 8), ce.squares(w, h, 9), ce.noise(w, h, 10)]
    kept = ce.ref_detect(imgs[1], 15, 0.01, 8.0)[0] + np.float32(0.25)
    masks = [cm.checker(w, h), cm.ref_disc_mask(w, h, kept, 6), None, np.zeros((h, w), np.uint8)]
    ctx.batch_configure(4, w, h, 1)
    for i, img in enumerate(imgs):
        ctx.batch_upload_image(i, padded(img))
    ctx.corners_batch_set_mask(0, padded(masks[0], 3))   # uploaded
    ctx.corners_batch_set_kept(1, kept, 6)               # built on the device
    ctx.corners_batch_set_mask(3, masks[3])              # all zero
    ctx.corners_batch_run(1, 3, 0, 0.01, 5.0, masked=True)
    for i in (3, 1, 2):
        want, n, _ = cm.ref_detect(imgs[i], masks[i], 0, 0.01, 5.0)
        got, m = ctx.corners_batch_get(i)
        assert m == n and np.array_equal(got, want), i
    assert ctx.corners_batch_get(3)[1] == 0
    ctx.corners_batch_run(0, 4, 30, 0.02, 10.5, masked=True)
    masked = [ctx.corners_batch_get(i) for i in range(4)]
    for i in range(4):
        want, n, _ = cm.ref_detect(imgs[i], masks[i], 30, 0.02, 10.5)
        assert masked[i][1] == n and np.array_equal(masked[i][0], want), i
    ctx.corners_batch_run(0, 4, 30, 0.02, 10.5)          # vocorn_batch_run: no masks
    plain = [ctx.corners_batch_get(i) for i in range(4)]
    assert np.array_equal(plain[2][0], masked[2][0]) and plain[2][1] == masked[2][1]   # the image without a mask: the same bytes
    assert not np.array_equal(plain[0][0], masked[0][0])
    for i in range(4):
        assert np.array_equal(plain[i][0], ce.ref_detect(imgs[i], 30, 0.02, 10.5)[0]), i
    ctx.corners_batch_set_mask(0, None)                  # removed: image 0 runs unmasked, image 1 still under its discs
    ctx.corners_batch_run(0, 2, 30, 0.02, 10.5, masked=True)
    assert np.array_equal(ctx.corners_batch_get(0)[0], plain[0][0]) and np.array_equal(ctx.corners_batch_get(1)[0], masked[1][0])
    ctx.corners_batch_set_kept(1, np.zeros((0, 2)), 6)   # no kept point: an all-255 mask, the unmasked corners
    ctx.corners_batch_run(1, 1, 30, 0.02, 10.5, masked=True)
    assert np.array_equal(ctx.corners_batch_get(1)[0], plain[1][0])
    ctx.corners_batch_set_mask(1, masks[0])
    ctx.batch_configure(4, w, h, 1)                      # drops every mask (the images stay)
    ctx.corners_batch_run(0, 4, 30, 0.02, 10.5, masked=True)
    for i in range(4):
        got, m = ctx.corners_batch_get(i)
        assert m == plain[i][1] and np.array_equal(got, plain[i][0]), i


def test_track_then_replenish_and_the_kept_image(volib, small_seq, small_world):
    c = volib.Context(0, 480, 160, 2048, 1)
    try:
        L, R = small_seq["L"], small_seq["R"]
        h, w = L[0].shape
        pts = small_seq["pts"][0][:300]
        before = c.flow_track(L[0], L[1], pts, win=15, min_eigenvals=True)
        nxt, st, _ = before
        ok = (st != 0) & (nxt[:, 0] >= 0) & (nxt[:, 0] <= w - 1) & (nxt[:, 1] >= 0) & (nxt[:, 1] <= h - 1)
        survivors = nxt[ok]
        assert 100 < len(survivors) <= 300
        target = 400
        want, n, _ = cm.ref_detect(L[1], cm.ref_disc_mask(w, h, survivors, 5), target - len(survivors), 0.01, 5.0)
        new = c.replenish_corners(L[1], survivors, 5, max_corners=target - len(survivors))
        assert len(new) == n and 0 < n <= target - len(survivors) and np.array_equal(new, want)
        centres = np.rint(survivors)
        d2 = ((new[:, None, :] - centres[None, :, :]) ** 2).sum(axis=2)
        assert d2.min() > 25, "every new corner lies more than 5 pixels from every rounded survivor"
        after = c.flow_track(L[0], L[1], pts, win=15, min_eigenvals=True)
        for a, b in zip(before, after):
            assert a.tobytes() == b.tobytes()   # the detector leaves the tracker's state alone
        # img == NULL: the left image of the kept pair, as in vocorn_detect
        n_out = C.c_int(0)
        mask = cm.left_half(w, h)
        assert c.lib.vocmask_detect(c.h, None, w, h, w, mask.ctypes.data, w, None, None, 0, C.byref(n_out)) == volib.VO_ERR_STATE
        assert c.lib.vocmask_replenish(c.h, None, w, h, w, survivors.ctypes.data, 5, 5, None, None, 0, C.byref(n_out)) == volib.VO_ERR_STATE
        P_l, P_r = small_world.proj_matrices()
        c.track_frame(L[0], R[0], L[1], R[1], small_seq["pts"][0], P_l, P_r)
        assert np.array_equal(c.good_features_to_track(None, 0, 0.01, 5.0, mask=mask), cm.ref_detect(L[1], mask, 0, 0.01, 5.0)[0])
        assert np.array_equal(c.replenish_corners(None, survivors, 5, 50), cm.ref_detect(L[1], cm.ref_disc_mask(w, h, survivors, 5), 50, 0.01, 5.0)[0])
        assert np.array_equal(c.good_features_to_track(None, 0, 0.01, 5.0), ce.ref_detect(L[1], 0, 0.01, 5.0)[0])   # ... still in place
    finally:
        c.close()


def test_errors_launch_nothing(volib):
    c = volib.Context(0, 128, 64, 64, 2)
    try:
        w, h = 64, 48
        lib, ARG, STATE = c.lib, volib.VO_ERR_ARG, volib.VO_ERR_STATE
        img, mask = ce.noise(w, h, 1), cm.checker(w, h)
        kept = np.array([(5.0, 5.0), (9.0, 20.0)], np.float32)
        out = np.zeros((h, w), np.uint8)
        n = C.c_int(-7)
        ip, mp, kp, op = img.ctypes.data, mask.ctypes.data, kept.ctypes.data, out.ctypes.data
        # without a configured table
        assert lib.vocmask_batch_set_mask(c.h, 0, mp, w) == STATE
        assert lib.vocmask_batch_set_kept(c.h, 0, kp, 2, 5) == STATE
        assert lib.vocmask_batch_run(c.h, None, 0, 1) == STATE
        assert b"vocmask" in lib.vo_last_error(c.h)
        # the synchronous calls
        assert lib.vocmask_detect(c.h, ip, w, h, w, mp, w - 1, None, None, 0, C.byref(n)) == ARG            # mask stride < w
        assert lib.vocmask_detect(c.h, ip, w, h, w - 1, mp, w, None, None, 0, C.byref(n)) == ARG            # image stride < w
        assert lib.vocmask_detect(c.h, ip, 16, 16, 16, mp, 16, None, None, 0, C.byref(n)) == ARG            # below 32 x 32
        assert lib.vocmask_detect(c.h, ip, w, h, w, mp, w, None, None, 0, None) == ARG
        assert lib.vocmask_detect(c.h, ip, w, h, w, mp, w, C.byref(volib.VoCornParams(0, 0.0, 5.0)), None, 0, C.byref(n)) == ARG
        for radius, nk, pk in ((-1, 2, kp), (257, 2, kp), (5, -1, kp), (5, 2, None), (5, 65, kp)):          # (max_pts is 64)
            assert lib.vocmask_replenish(c.h, ip, w, h, w, pk, nk, radius, None, None, 0, C.byref(n)) == ARG, (radius, nk)
            assert lib.vocmask_disc_mask(c.h, w, h, pk, nk, radius, op, w) == ARG, (radius, nk)
        assert lib.vocmask_disc_mask(c.h, w, h, kp, 2, 5, op, w - 1) == ARG
        assert lib.vocmask_disc_mask(c.h, w, h, kp, 2, 5, None, w) == ARG
        assert lib.vocmask_disc_mask(c.h, 16, 16, kp, 2, 5, op, 16) == ARG
        assert n.value == -7 and not out.any()
        # the batch calls
        c.batch_configure(3, w, h, 1)
        for idx in (-1, 3):
            assert lib.vocmask_batch_set_mask(c.h, idx, mp, w) == ARG
            assert lib.vocmask_batch_set_kept(c.h, idx, kp, 2, 5) == ARG
        assert lib.vocmask_batch_set_mask(c.h, 0, mp, w - 1) == ARG
        for radius, nk, pk in ((-1, 2, kp), (257, 2, kp), (5, -1, kp), (5, 2, None), (5, 65, kp)):
            assert lib.vocmask_batch_set_kept(c.h, 0, pk, nk, radius) == ARG, (radius, nk)
        assert lib.vocmask_batch_run(c.h, None, 2, 2) == ARG and lib.vocmask_batch_run(c.h, None, -1, 1) == ARG
        assert lib.vocmask_batch_run(c.h, C.byref(volib.VoCornParams(0, 0.01, 256.5)), 0, 1) == ARG
        assert lib.vocmask_batch_set_mask(c.h, 0, None, 0) == 0                                             # nothing to remove
        # inside the sequence loop every entry refuses
        c.seq_configure(1, w, h)
        assert lib.vocmask_detect(c.h, ip, w, h, w, mp, w, None, None, 0, C.byref(n)) == STATE
        assert lib.vocmask_disc_mask(c.h, w, h, kp, 2, 5, op, w) == STATE
        assert lib.vocmask_replenish(c.h, ip, w, h, w, kp, 2, 5, None, None, 0, C.byref(n)) == STATE
        assert lib.vocmask_batch_set_mask(c.h, 0, mp, w) == STATE
        assert lib.vocmask_batch_set_kept(c.h, 0, kp, 2, 5) == STATE
        assert lib.vocmask_batch_run(c.h, None, 0, 1) == STATE
        assert b"sequence loop" in lib.vo_last_error(c.h)
    finally:
        c.close()


def test_context_that_never_calls_vocmask_equals_the_unmasked_emulator(volib):
    c = volib.Context(0, 160, 96, 64, 1)
    try:
        img = ce.noise(131, 67, 4)
        want = ce.emu_detect([img], 0, 0.01, 5.0)[0]
        got = c.good_features_to_track(img, 0, 0.01, 5.0)
        assert len(got) == want[1] and got.tobytes() == want[0].tobytes()
    finally:
        c.close()
