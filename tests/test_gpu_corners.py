"""The Shi-Tomasi detector of include/vo_corners.h on the device, held BIT FOR BIT -- the quality map and the corner lists with their
order; identity, as for FAST corners, no tolerance -- to the restatement of OpenCV in tests/host_check/corners_ref.c, over the case
table of the emulator tests at the sizes a context takes (32 x 32 and up; the smaller shapes run in test_corners_emulation.py):
vocorn_min_eigen_map, vocorn_detect and vocorn_batch_*."""
import ctypes as C

import numpy as np
import pytest

import corners_emu as ce

pytestmark = pytest.mark.gpu

SHAPES = [(32, 32), (33, 35), (64, 32), (65, 33), (131, 67)]   # one tile, partial tiles both ways, exact tiles, 3 x 5 tiles
CONTENTS = [("noise", lambda w, h: ce.noise(w, h, 1)), ("blobs", lambda w, h: ce.blobs(w, h, 2)), ("squares", lambda w, h: ce.squares(w, h, 3)),
            ("periodic", lambda w, h: ce.periodic(w, h)), ("border_max", ce.border_max),
            ("dark_highlights", lambda w, h: ce.dark_highlights(w, h, 5))]
DISTANCES = [0.0, 1.0, 5.0, 10.5, 32.0]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def ctx(volib):
    c = volib.Context(0, 256, 128, 256, 4)
    yield c
    c.close()


def padded(img, extra=5):
    """the image as a view of a wider array: a byte stride that is not the width"""
    h, w = img.shape
    buf = np.full((h, w + extra), 0xEE, np.uint8)
    buf[:, :w] = img
    return buf[:, :w]


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_map_and_corners_bit_for_bit(ctx, shape):
    w, h = shape
    for name, gen in CONTENTS:
        img = gen(w, h)
        assert np.array_equal(bits(ctx.corner_min_eigen_val(padded(img))), bits(ce.ref_map(img))), name   # border pixels included
        for md in DISTANCES:
            want, n, _ = ce.ref_detect(img, 0, 0.01, md)
            got = ctx.good_features_to_track(padded(img), 0, 0.01, md)
            assert len(got) == n and np.array_equal(got, want), (name, md)


def test_adversarial_contents(ctx, volib):
    img = ce.noise(33, 35, 2)           # one-sided border: the ref with the trap on differs, the device must not
    assert not np.array_equal(ce.ref_map(img), ce.ref_map(img, trap=1))
    assert np.array_equal(bits(ctx.corner_min_eigen_val(img)), bits(ce.ref_map(img)))
    assert np.array_equal(ctx.good_features_to_track(img, 0, 0.05, 0.0), ce.ref_detect(img, 0, 0.05, 0.0)[0])
    img = ce.dark_highlights(131, 67, 0)   # the box filter's summation order is part of the result here (the ref can do both)
    assert not np.array_equal(bits(ce.ref_map(img)), bits(ce.ref_map(img, order=1)))
    assert np.array_equal(bits(ctx.corner_min_eigen_val(img)), bits(ce.ref_map(img)))
    assert np.array_equal(ctx.good_features_to_track(img, 0, 0.01, 5.0), ce.ref_detect(img, 0, 0.01, 5.0)[0])
    img = ce.chain(200, 33, 44, 4)      # the dependency chain: 44 rounds deep
    want, n, nc = ce.ref_detect(img, 0, 0.01, 6.0)
    assert (n, nc) == (22, 44) and np.array_equal(ctx.good_features_to_track(img, 0, 0.01, 6.0), want)
    img = ce.noise(131, 67, 4)          # max_corners binding, with and without suppression; cap < n
    full, n, _ = ce.ref_detect(img, 0, 0.01, 5.0)
    for mc, md in ((1, 5.0), (17, 5.0), (n, 5.0), (n + 5, 5.0), (17, 0.0)):
        assert np.array_equal(ctx.good_features_to_track(img, mc, 0.01, md), ce.ref_detect(img, mc, 0.01, md)[0]), (mc, md)
    pts = np.full((9, 2), -1, np.float32)
    cnt = C.c_int(0)
    prm = volib.VoCornParams(0, 0.01, 5.0)
    assert ctx.lib.vocorn_detect(ctx.h, img.ctypes.data, 131, 67, 131, C.byref(prm), pts.ctypes.data, 9, C.byref(cnt)) == 0
    assert cnt.value == n and np.array_equal(pts, full[:9])
    assert ctx.lib.vocorn_detect(ctx.h, img.ctypes.data, 131, 67, 131, None, None, 0, C.byref(cnt)) == 0   # NULL params: the defaults
    assert cnt.value == ce.ref_detect(img, 5000, 0.01, 5.0)[1]


def test_batch_of_three_images_and_a_range_that_starts_at_one(ctx):
    w, h = 131, 67
    imgs = [ce.noise(w, h, 7), ce.blobs(w, h, 8), ce.squares(w, h, 9), ce.periodic(w, h)]
    ctx.batch_configure(4, w, h, 1)
    for i, img in enumerate(imgs):
        ctx.batch_upload_image(i, padded(img))
    ctx.corners_batch_run(1, 3, 0, 0.01, 5.0)
    for i in (3, 1, 2):
        want, n, _ = ce.ref_detect(imgs[i], 0, 0.01, 5.0)
        got, m = ctx.corners_batch_get(i)
        assert m == n and np.array_equal(got, want), i
    ctx.corners_batch_run(0, 4, 30, 0.02, 10.5)
    for i in range(4):
        want, n, _ = ce.ref_detect(imgs[i], 30, 0.02, 10.5)
        got, m = ctx.corners_batch_get(i, cap=7)
        assert m == n and np.array_equal(got, want[:7]), i
    n = C.c_int(0)
    ctx.corners_batch_run(1, 2)
    assert ctx.lib.vocorn_batch_get(ctx.h, 0, None, 0, C.byref(n)) == ctx.lib.vocorn_batch_get(ctx.h, 3, None, 0, C.byref(n)) == -1   # outside the run
    assert ctx.lib.vocorn_batch_run(ctx.h, None, 2, 3) == -1 and ctx.lib.vocorn_batch_run(ctx.h, None, -1, 1) == -1                     # outside the table
    ctx.batch_configure(2, w, h, 1)
    assert ctx.lib.vocorn_batch_get(ctx.h, 1, None, 0, C.byref(n)) == -3                                                               # another table: VO_ERR_STATE


def test_colour_formats_equal_the_gray_call_on_the_converted_image(volib):
    from test_gpu_ingest_formats import FORMATS, GRAY8_X2, colourise, to_gray
    c = volib.Context(0, 256, 128, 256, 1)
    try:
        gray = ce.blobs(131, 67, 11)
        for fmt in FORMATS:
            if fmt == GRAY8_X2:
                frame = np.ascontiguousarray(np.stack([gray, ce.noise(131, 67, 12)], axis=-1))
                img, conv = frame[..., 0], frame[..., 0].copy()
            else:
                img = colourise(gray, fmt, 13)
                conv = to_gray(img, fmt)
            c.set_params(input_format=fmt)
            got, eig = c.good_features_to_track(img, 0, 0.01, 5.0), c.corner_min_eigen_val(img)
            c.set_params(input_format=0)
            assert np.array_equal(got, c.good_features_to_track(conv, 0, 0.01, 5.0)), fmt
            assert np.array_equal(got, ce.ref_detect(conv, 0, 0.01, 5.0)[0]), fmt
            assert np.array_equal(bits(eig), bits(ce.ref_map(conv))), fmt
    finally:
        c.close()


def test_kept_pair_errors_and_the_tracker_beside_the_detector(volib, small_seq, small_world):
    c = volib.Context(0, 480, 160, 2048, 1)
    try:
        L, R = small_seq["L"], small_seq["R"]
        h, w = L[0].shape
        n = C.c_int(0)
        prm = volib.VoCornParams(0, 0.01, 5.0)
        eig = np.zeros((h, w), np.float32)
        # no kept pair yet: VO_ERR_STATE, with text
        assert c.lib.vocorn_detect(c.h, None, w, h, w, C.byref(prm), None, 0, C.byref(n)) == volib.VO_ERR_STATE
        assert c.lib.vocorn_min_eigen_map(c.h, None, w, h, w, eig.ctypes.data, w) == volib.VO_ERR_STATE
        assert c.lib.vo_last_error(c.h)
        P_l, P_r = small_world.proj_matrices()
        c.track_frame(L[0], R[0], L[1], R[1], small_seq["pts"][0], P_l, P_r)
        want = ce.ref_detect(L[1], 0, 0.01, 5.0)[0]
        assert np.array_equal(c.good_features_to_track(None, 0, 0.01, 5.0), want)          # img == NULL: the kept pair's left image
        assert np.array_equal(c.good_features_to_track(L[1], 0, 0.01, 5.0), want)
        assert np.array_equal(bits(c.corner_min_eigen_val(None)), bits(ce.ref_map(L[1])))
        assert np.array_equal(c.good_features_to_track(None, 0, 0.01, 5.0), want)          # ... which a call with an image left in place
        # the documented argument errors; nothing is launched
        img = L[0]
        bad = [volib.VoCornParams(0, 0.0, 5.0), volib.VoCornParams(0, float("nan"), 5.0), volib.VoCornParams(0, 0.01, -1.0),
               volib.VoCornParams(-1, 0.01, 5.0), volib.VoCornParams(0, 0.01, 256.5)]
        for p in bad:
            assert c.lib.vocorn_detect(c.h, img.ctypes.data, w, h, w, C.byref(p), None, 0, C.byref(n)) == volib.VO_ERR_ARG
            assert c.lib.vocorn_batch_run(c.h, C.byref(p), 0, 1) == volib.VO_ERR_ARG
        assert c.lib.vocorn_detect(c.h, img.ctypes.data, w, h, w - 1, C.byref(prm), None, 0, C.byref(n)) == volib.VO_ERR_ARG   # stride < width
        assert c.lib.vocorn_detect(c.h, img.ctypes.data, 16, 16, 16, C.byref(prm), None, 0, C.byref(n)) == volib.VO_ERR_ARG    # below 32 x 32
        assert c.lib.vocorn_detect(c.h, img.ctypes.data, w, h, w, C.byref(prm), None, 0, None) == volib.VO_ERR_ARG
        assert c.lib.vocorn_detect(c.h, img.ctypes.data, w, h, w, C.byref(prm), None, 5, C.byref(n)) == volib.VO_ERR_ARG
        assert c.lib.vocorn_min_eigen_map(c.h, img.ctypes.data, w, h, w, eig.ctypes.data, w - 1) == volib.VO_ERR_ARG
        assert c.lib.vocorn_min_eigen_map(c.h, img.ctypes.data, w, h, w, None, w) == volib.VO_ERR_ARG
        assert c.lib.vocorn_batch_get(c.h, 0, None, 0, C.byref(n)) == volib.VO_ERR_STATE                                     # no batch run
        assert b"vocorn" in c.lib.vo_last_error(c.h)
        # a voflag_track right after a detect gives the bytes it gave before: the detector leaves the tracker's state alone
        pts = small_seq["pts"][0][:200]
        before = c.flow_track(L[0], L[1], pts, win=15, min_eigenvals=True)
        c.good_features_to_track(L[0], 100, 0.01, 5.0)
        after = c.flow_track(L[0], L[1], pts, win=15, min_eigenvals=True)
        for a, b in zip(before, after):
            assert a.tobytes() == b.tobytes()
        c2 = volib.Context(0, 512, 320, 16, 2)
        try:
            assert c2.lib.vocorn_batch_run(c2.h, None, 0, 1) == volib.VO_ERR_STATE   # no table configured
            # more candidates than the corner-list capacity (16 384 in this context): VO_ERR_OVERFLOW, nothing written
            dots = ce.periodic(512, 320, 4)
            assert ce.ref_detect(dots, 0, 1e-6, 0.0, cap=0)[2] > 16384
            out = np.full((8, 2), -5, np.float32)
            n.value = -77
            p = volib.VoCornParams(0, 1e-6, 0.0)
            assert c2.lib.vocorn_detect(c2.h, dots.ctypes.data, 512, 320, 512, C.byref(p), out.ctypes.data, 8, C.byref(n)) == volib.VO_ERR_OVERFLOW
            assert n.value == -77 and (out == -5).all() and b"capacity" in c2.lib.vo_last_error(c2.h)
            c2.batch_configure(2, 512, 320, 1)
            c2.batch_upload_image(0, dots)
            c2.batch_upload_image(1, ce.blobs(512, 320, 3, count=40))
            c2.corners_batch_run(0, 2, 0, 1e-6, 0.0)
            assert c2.lib.vocorn_batch_get(c2.h, 0, out.ctypes.data, 8, C.byref(n)) == volib.VO_ERR_OVERFLOW and (out == -5).all()
            got, m = c2.corners_batch_get(1)   # the other image of the run is not affected
            want = ce.ref_detect(ce.blobs(512, 320, 3, count=40), 0, 1e-6, 0.0)
            assert m == want[1] and np.array_equal(got, want[0][:len(got)])
            # inside the sequence loop every entry refuses
            c2.seq_configure(1, 512, 320)
            eig2 = np.zeros((320, 512), np.float32)
            assert c2.lib.vocorn_detect(c2.h, dots.ctypes.data, 512, 320, 512, None, None, 0, C.byref(n)) == volib.VO_ERR_STATE
            assert c2.lib.vocorn_min_eigen_map(c2.h, dots.ctypes.data, 512, 320, 512, eig2.ctypes.data, 512) == volib.VO_ERR_STATE
            assert c2.lib.vocorn_batch_run(c2.h, None, 0, 1) == volib.VO_ERR_STATE
            assert c2.lib.vocorn_batch_get(c2.h, 0, None, 0, C.byref(n)) == volib.VO_ERR_STATE
            assert b"sequence loop" in c2.lib.vo_last_error(c2.h)
        finally:
            c2.close()
    finally:
        c.close()
