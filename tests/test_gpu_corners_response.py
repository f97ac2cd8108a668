"""The Shi-Tomasi detector with a response (include/vo_corners_response.h) on the device, held BIT FOR BIT -- response maps, and corner
lists with their order; identity, no tolerance -- to tests/host_check/corners_response_ref.c: voresp_map, voresp_detect and
voresp_batch_run at (5, min-eigen), (3, Harris) and (5, Harris), over the content generators, the widths around the B = 5 column
split, the adversarial images, the mask calls, the default-parameter identity with vocorn_* / vocmask_*, the errors, the kept pair
and a seeded fuzz."""
import ctypes as C

import numpy as np
import pytest

import corners_emu as ce
import corners_mask_cases as cm
import corners_response_cases as cr
import corners_response_fuzz_cases as fz

pytestmark = pytest.mark.gpu

SHAPES = [(32, 32), (33, 35), (65, 33), (131, 67)]
RESP_IDS = ["B%d-%s" % (b, "harris" if hr else "mineig") for b, hr in cr.RESPONSES]


@pytest.fixture(scope="module")
def ctx(volib):
    c = volib.Context(0, 512, 192, 256, 4)
    yield c
    c.close()


def padded(a, extra=5):
    """the array as a view of a wider one: a byte stride that is not the width"""
    h, w = a.shape
    buf = np.full((h, w + extra), 0xEE, np.uint8)
    buf[:, :w] = a
    return buf[:, :w]


def detect(ctx, img, mask, mc, q, md, block, harris, k=cr.K):
    return ctx.good_features_to_track(img, mc, q, md, mask=mask, block_size=block, use_harris=harris, k=k)


@pytest.mark.parametrize("block,harris", cr.RESPONSES, ids=RESP_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_maps_and_lists_bit_for_bit(ctx, shape, block, harris):
    w, h = shape
    for name, _ in cr.CONTENTS:
        img = cr.content(name, w, h)
        got = ctx.corner_response_map(padded(img), block, harris, cr.K)
        assert np.array_equal(cr.bits(got), cr.bits(cr.expected_map(name, w, h, block, harris))), name
        for md in cr.DISTANCES:
            want, n, _ = cr.expected(name, w, h, block, harris, md)
            got = detect(ctx, padded(img), None, 0, 0.01, md, block, harris)
            assert len(got) == n and got.tobytes() == want.tobytes(), (name, md)
    want = cr.expected("noise", w, h, block, harris, 5.0, cr.K, 0.01, 17)
    assert detect(ctx, cr.content("noise", w, h), None, 17, 0.01, 5.0, block, harris).tobytes() == want[0].tobytes()


@pytest.mark.parametrize("w", cr.SEAM_WIDTHS)
def test_widths_around_the_block_5_column_split(ctx, w):
    """one below the 252 columns a workgroup of the B = 5 map kernel owns, exactly that many, one above, two workgroups' worth"""
    h = 32
    img = ce.noise(w, h, 61)
    for block, harris in cr.RESPONSES:
        assert np.array_equal(cr.bits(ctx.corner_response_map(img, block, harris)), cr.bits(cr.ref_map(img, block, harris))), (block, harris)
        want, n, _ = cr.ref_detect(img, None, 0, 0.01, 5.0, block, harris)
        got = detect(ctx, img, None, 0, 0.01, 5.0, block, harris)
        assert len(got) == n and got.tobytes() == want.tobytes(), (block, harris)


def test_adversarial_contents(ctx):
    for block in (3, 5):
        for harris in (0, 1):
            if (block, harris) == (3, 0):
                continue
            trap = cr.one_sided(65, 33, 6)                            # the trap image: reflected cov, not cov of the reflected source
            assert np.array_equal(cr.bits(ctx.corner_response_map(trap, block, harris)), cr.bits(cr.ref_map(trap, block, harris)))
            dark = ce.dark_highlights(131, 67, 2)                     # the order-sensitive image: the running column sum
            assert np.array_equal(cr.bits(ctx.corner_response_map(dark, block, harris)), cr.bits(cr.ref_map(dark, block, harris)))
            want, n, _ = cr.ref_detect(dark, None, 0, 0.01, 5.0, block, harris)
            got = detect(ctx, dark, None, 0, 0.01, 5.0, block, harris)
            assert len(got) == n and got.tobytes() == want.tobytes()
        ramp = cr.ramp(32, 32)                                        # the negative maximum, at both quality levels
        m = ctx.corner_response_map(ramp, block, 1)
        assert (m < 0).all() and np.array_equal(cr.bits(m), cr.bits(cr.ref_map(ramp, block, 1)))
        assert len(detect(ctx, ramp, None, 0, 0.01, 0.0, block, 1)) == 0
        for md in (0.0, 5.0):
            want, n, _ = cr.ref_detect(ramp, None, 0, 3.0, md, block, 1)
            got = detect(ctx, ramp, None, 0, 3.0, md, block, 1)
            assert len(got) == n and got.tobytes() == want.tobytes(), md
            assert md > 0 or n == 840
        want, n, _ = cr.ref_detect(ramp, cm.left_half(32, 32), 0, 3.0, 2.0, block, 1)
        assert detect(ctx, ramp, cm.left_half(32, 32), 0, 3.0, 2.0, block, 1).tobytes() == want.tobytes()
        img = ce.noise(131, 67, 5)
        for k in cr.HARRIS_KS:                                        # k = 0, a negative k, k = 0.25
            assert np.array_equal(cr.bits(ctx.corner_response_map(img, block, 1, k)), cr.bits(cr.ref_map(img, block, 1, k))), k
            want, n, _ = cr.ref_detect(img, None, 0, 0.01, 5.0, block, 1, k)
            got = detect(ctx, img, None, 0, 0.01, 5.0, block, 1, k)
            assert len(got) == n and got.tobytes() == want.tobytes(), k


@pytest.mark.parametrize("block,harris", cr.RESPONSES, ids=RESP_IDS)
def test_with_the_mask_calls(ctx, block, harris):
    w, h = 131, 67
    for name, img, mask, mc, q, md in cm.mask_cases(w, h):            # under an uploaded mask
        want, n, _ = cr.ref_detect(img, mask, mc, q, md, block, harris)
        got = detect(ctx, padded(img), padded(mask, 9), mc, q, md, block, harris)
        assert len(got) == n and got.tobytes() == want.tobytes(), name
    imgs = [ce.noise(w, h, 7), ce.blobs(w, h, 8), ce.squares(w, h, 9), ce.noise(w, h, 10)]
    kept = ce.ref_detect(imgs[1], 15, 0.01, 8.0)[0] + np.float32(0.25)
    masks = [cm.checker(w, h), cm.ref_disc_mask(w, h, kept, 6), None, cm.left_half(w, h)]
    ctx.batch_configure(4, w, h, 1)
    for i, img in enumerate(imgs):
        ctx.batch_upload_image(i, padded(img))
    ctx.corners_batch_set_mask(0, masks[0])
    ctx.corners_batch_set_kept(1, kept, 6)                            # discs built on the device
    ctx.corners_batch_set_mask(3, padded(masks[3], 3))
    ctx.corners_batch_run(1, 3, 0, 0.01, 5.0, block_size=block, use_harris=harris)   # a batch of three whose range starts at one
    for i in (3, 1, 2):
        want, n, _ = cr.ref_detect(imgs[i], masks[i], 0, 0.01, 5.0, block, harris)
        got, m = ctx.corners_batch_get(i)
        assert m == n and got.tobytes() == want.tobytes(), i
    ctx.corners_batch_run(0, 4, 30, 0.02, 10.5, masked=True)          # vocmask_batch_run afterwards: the 3 x 3 minimum eigenvalue again
    for i in range(4):
        want, n, _ = cm.ref_detect(imgs[i], masks[i], 30, 0.02, 10.5)
        got, m = ctx.corners_batch_get(i)
        assert m == n and np.array_equal(got, want), i


def test_default_params_are_the_other_two_headers_byte_for_byte(ctx, volib):
    w, h = 131, 67
    img, mask = ce.noise(w, h, 3), cm.checker(w, h)
    lib = ctx.lib
    dflt = volib.VoRespParams(3, 0, 0.04)
    prm = volib.VoCornParams(0, 0.01, 5.0)
    for rsp in (None, C.byref(dflt)):
        for m in (None, mask):
            pts = np.full((w * h, 2), -5.0, np.float32)
            n = C.c_int(-1)
            assert lib.voresp_detect(ctx.h, img.ctypes.data, w, h, w, None if m is None else m.ctypes.data, w, C.byref(prm), rsp, pts.ctypes.data, w * h,
                                     C.byref(n)) == 0
            want = ctx.good_features_to_track(img, 0, 0.01, 5.0, mask=m)   # vocorn_detect / vocmask_detect
            assert n.value == len(want) and pts[:n.value].tobytes() == want.tobytes() and (pts[n.value:] == -5.0).all()
        out = np.zeros((h, w + 3), np.float32)
        assert lib.voresp_map(ctx.h, img.ctypes.data, w, h, w, rsp, out.ctypes.data, w + 3) == 0
        assert out[:, :w].tobytes() == ctx.corner_min_eigen_val(img).tobytes() and not out[:, w:].any()
    ctx.batch_configure(2, w, h, 1)
    ctx.batch_upload_image(0, img)
    ctx.batch_upload_image(1, ce.blobs(w, h, 4))
    ctx.corners_batch_set_mask(1, mask)
    ctx.corners_batch_run(0, 2, 0, 0.01, 5.0, masked=True)
    want = [ctx.corners_batch_get(i) for i in range(2)]
    assert lib.voresp_batch_run(ctx.h, C.byref(prm), None, 0, 2) == 0
    for i in range(2):
        got, n = ctx.corners_batch_get(i)
        assert n == want[i][1] and got.tobytes() == want[i][0].tobytes()


def test_errors_and_the_next_valid_call(volib):
    c = volib.Context(0, 128, 64, 64, 2)
    try:
        w, h = 64, 48
        lib, ARG, STATE = c.lib, volib.VO_ERR_ARG, volib.VO_ERR_STATE
        img = ce.noise(w, h, 1)
        before = detect(c, img, None, 0, 0.01, 5.0, 5, 1)
        before_map = c.corner_response_map(img, 5, 1)
        assert before.tobytes() == cr.ref_detect(img, None, 0, 0.01, 5.0, 5, 1)[0].tobytes()
        pts = np.full((w * h, 2), -5.0, np.float32)
        out = np.full((h, w), -5.0, np.float32)
        n = C.c_int(-7)
        bad = [(1, 0, 0.04), (4, 0, 0.04), (7, 0, 0.04), (0, 0, 0.04), (-3, 1, 0.04), (3, 2, 0.04), (5, -1, 0.04), (5, 1, float("nan")), (3, 0, float("inf")),
               (5, 1, float("-inf"))]
        c.batch_configure(2, w, h, 1)
        c.batch_upload_image(0, img)
        for b, hr, k in bad:
            r = volib.VoRespParams(b, hr, k)
            assert lib.voresp_detect(c.h, img.ctypes.data, w, h, w, None, 0, None, C.byref(r), pts.ctypes.data, w * h, C.byref(n)) == ARG, (b, hr, k)
            assert b"block_size 3 and 5" in lib.vo_last_error(c.h)
            assert lib.voresp_map(c.h, img.ctypes.data, w, h, w, C.byref(r), out.ctypes.data, w) == ARG, (b, hr, k)
            assert lib.voresp_batch_run(c.h, None, C.byref(r), 0, 1) == ARG, (b, hr, k)
        assert n.value == -7 and (pts == -5.0).all() and (out == -5.0).all()
        good = volib.VoRespParams(5, 1, 0.04)
        assert lib.voresp_batch_run(c.h, None, C.byref(good), 1, 2) == ARG                                   # a range outside the table
        assert lib.voresp_batch_run(c.h, C.byref(volib.VoCornParams(0, 0.0, 5.0)), C.byref(good), 0, 1) == ARG
        assert lib.voresp_detect(c.h, img.ctypes.data, w, h, w, None, 0, None, C.byref(good), pts.ctypes.data, w * h, None) == ARG
        assert lib.voresp_detect(c.h, img.ctypes.data, w, h, w, img.ctypes.data, w - 1, None, C.byref(good), pts.ctypes.data, w * h, C.byref(n)) == ARG
        assert lib.voresp_detect(c.h, img.ctypes.data, 16, 16, 16, None, 0, None, C.byref(good), pts.ctypes.data, w * h, C.byref(n)) == ARG
        assert lib.voresp_map(c.h, img.ctypes.data, w, h, w, C.byref(good), out.ctypes.data, w - 1) == ARG
        assert lib.voresp_map(c.h, img.ctypes.data, w, h, w, C.byref(good), None, w) == ARG
        # the next valid call gives the bytes it gave before
        assert detect(c, img, None, 0, 0.01, 5.0, 5, 1).tobytes() == before.tobytes()
        assert c.corner_response_map(img, 5, 1).tobytes() == before_map.tobytes()
        # without a configured table (the synchronous calls took it), and inside the sequence loop
        c2 = volib.Context(0, 128, 64, 64, 2)
        try:
            assert c2.lib.voresp_batch_run(c2.h, None, C.byref(good), 0, 1) == STATE
            assert b"voresp_batch_run" in c2.lib.vo_last_error(c2.h)
        finally:
            c2.close()
        c.seq_configure(1, w, h)
        assert lib.voresp_detect(c.h, img.ctypes.data, w, h, w, None, 0, None, C.byref(good), pts.ctypes.data, w * h, C.byref(n)) == STATE
        assert lib.voresp_map(c.h, img.ctypes.data, w, h, w, C.byref(good), out.ctypes.data, w) == STATE
        assert lib.voresp_batch_run(c.h, None, C.byref(good), 0, 1) == STATE
        assert b"sequence loop" in lib.vo_last_error(c.h)
    finally:
        c.close()


def test_the_kept_image(volib, small_seq, small_world):
    c = volib.Context(0, 480, 160, 2048, 1)
    try:
        L, R = small_seq["L"], small_seq["R"]
        h, w = L[0].shape
        n_out = C.c_int(0)
        good = volib.VoRespParams(5, 1, 0.04)
        out = np.zeros((h, w), np.float32)
        assert c.lib.voresp_detect(c.h, None, w, h, w, None, 0, None, C.byref(good), None, 0, C.byref(n_out)) == volib.VO_ERR_STATE
        assert c.lib.voresp_map(c.h, None, w, h, w, C.byref(good), out.ctypes.data, w) == volib.VO_ERR_STATE
        P_l, P_r = small_world.proj_matrices()
        c.track_frame(L[0], R[0], L[1], R[1], small_seq["pts"][0], P_l, P_r)
        mask = cm.left_half(w, h)
        for block, harris in cr.RESPONSES:
            assert np.array_equal(cr.bits(c.corner_response_map(None, block, harris)), cr.bits(cr.ref_map(L[1], block, harris)))
            assert detect(c, None, None, 0, 0.01, 5.0, block, harris).tobytes() == cr.ref_detect(L[1], None, 0, 0.01, 5.0, block, harris)[0].tobytes()
            assert detect(c, None, mask, 50, 0.01, 5.0, block, harris).tobytes() == cr.ref_detect(L[1], mask, 50, 0.01, 5.0, block, harris)[0].tobytes()
    finally:
        c.close()


def test_seeded_fuzz_of_60(ctx):
    cases = fz.cases()
    assert len(cases) == 60
    ran = 0
    for i, c in enumerate(cases):
        wmap, wpts, n = fz.expected(c)
        img = c["img"]                                                # a view: stride 160
        assert np.array_equal(cr.bits(ctx.corner_response_map(img, c["block"], c["harris"], c["k"])), cr.bits(wmap)), i
        mask = None if c["mask"] is None else padded(c["mask"], 9)
        got = ctx.good_features_to_track(img, c["mc"], c["q"], c["md"], mask=mask, block_size=c["block"], use_harris=c["harris"], k=c["k"])
        assert len(got) == n and got.tobytes() == wpts.tobytes(), (i, c["block"], c["harris"], c["k"], c["md"], c["q"], c["mc"], img.shape)
        ran += 1
    assert ran == 60
