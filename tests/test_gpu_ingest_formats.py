"""Input formats on the MI355X (-m gpu): colour and interleaved stereo frames handed to the library as they are
(vo_params.input_format, VO_FMT_*) against the SAME calls of a VO_FMT_GRAY8 context fed with images converted on the host by a
few lines of numpy written here (the integer formula of include/vo_hip.h; plane slicing for the two-byte interleave).  Every
comparison is bit for bit -- pixels, every output array, count, status, rvec / tvec, trajectory rows and info.

The colour inputs are built so that the three channels DIFFER (gains, offsets and noise per channel, clipped): a conversion
that picks one channel, swaps B and R or drops the rounding term fails.  Schedules are pinned in both contexts of a comparison
(a schedule never changes a result; pinning only skips the probes' time)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GRAY8, GRAY8_X2, BGR8, RGB8, BGRA8, RGBA8 = 0, 1, 2, 3, 4, 5
BPP = {GRAY8: 1, GRAY8_X2: 2, BGR8: 3, RGB8: 3, BGRA8: 4, RGBA8: 4}
NAMES = {GRAY8_X2: "gray8_x2", BGR8: "bgr8", RGB8: "rgb8", BGRA8: "bgra8", RGBA8: "rgba8"}
FORMATS = sorted(NAMES)
fmt_param = pytest.mark.parametrize("fmt", FORMATS, ids=lambda f: NAMES[f])


def to_gray(px, fmt):
    """the comparator's host conversion: (h, w, 3 | 4) uint8 in the format's channel order -> (h, w) uint8"""
    p = px.astype(np.int64)
    b, g, r = (p[..., 0], p[..., 1], p[..., 2]) if fmt in (BGR8, BGRA8) else (p[..., 2], p[..., 1], p[..., 0])
    return ((b * 1868 + g * 9617 + r * 4899 + 8192) >> 14).astype(np.uint8)


def colourise(gray, fmt, seed):
    """a colour image of the format's layout whose channels differ from each other and from `gray`"""
    rng = np.random.default_rng(seed)
    g = gray.astype(np.float64)
    chans = [np.clip(g * 0.85 + 40 + rng.integers(-6, 7, g.shape), 0, 255),     # B
             np.clip(g * 1.05 - 9 + rng.integers(-4, 5, g.shape), 0, 255),      # G
             np.clip(g * 0.70 + 25 + rng.integers(-9, 10, g.shape), 0, 255)]    # R
    if fmt in (RGB8, RGBA8):
        chans = chans[::-1]
    if BPP[fmt] == 4:
        chans.append(rng.integers(0, 256, g.shape))                               # alpha: ignored
    return np.ascontiguousarray(np.stack(chans, axis=-1).astype(np.uint8))


def encode_pair(left, right, fmt, seed):
    """one stereo pair as a context of format `fmt` takes it -> (left array, right array, left gray, right gray, owner); the
    grays are numpy's conversion of exactly those arrays"""
    if fmt == GRAY8_X2:   # the sensor's frame: one 16-bit word per pixel, left = low byte, right = high byte
        frame = np.ascontiguousarray(np.stack([left, right], axis=-1))
        return frame[..., 0], frame[..., 1], frame[..., 0].copy(), frame[..., 1].copy(), frame
    cl, cr = colourise(left, fmt, seed), colourise(right, fmt, seed + 1)
    return cl, cr, to_gray(cl, fmt), to_gray(cr, fmt), (cl, cr)


def pinned_schedule(ctx):
    ctx.set_schedule(pose_waves=2, pose_streams=1, prepare=0, epnp_wide_frames=4)


def same(a, b, what):
    if isinstance(a, dict):
        assert a.keys() == b.keys(), what
        for k in a:
            same(a[k], b[k], (what, k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            same(x, y, (what, i))
    elif isinstance(a, np.ndarray):
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), what
    else:
        assert a == b, what


@pytest.fixture(scope="module")
def small4(small_world):
    L, R, _, _ = small_world.render_sequence(4)
    return L, R


@pytest.fixture(scope="module")
def vga_pair():
    from visual_odom_amd import synth
    world = synth.StereoWorld(seed=31, width=640, height=480, fx=420.0, cx=319.5, cy=239.5, bf=-220.0, tex_size=1024)
    L, R, _, _ = world.render_sequence(2)
    return L, R, world.proj_matrices()


# ------------------------------------------------------------------ batch upload: level 0 is numpy's gray image
@fmt_param
def test_batch_upload_host_and_device(volib, small4, kitti_seq, vga_pair, fmt):
    import torch
    dev = torch.device("cuda", 0)
    cases = [(small4[0][0], small4[1][0]), (vga_pair[0][0], vga_pair[1][0]), (kitti_seq["L"][0], kitti_seq["R"][0])]
    for left, right in cases:
        h, w = left.shape
        a, b, ga, gb, owner = encode_pair(left, right, fmt, 5)
        ctx = volib.Context(0, w, h, 64, 1)
        try:
            ctx.set_params(input_format=fmt)
            assert ctx.get_params().input_format == fmt
            ctx.batch_configure(4, w, h, 1)
            ctx.batch_upload_image(0, a)
            ctx.batch_upload_image(1, b)
            # a padded host buffer: raw rows with a stride
            pad = np.full((h, w * BPP[fmt] + 19), 0xEE, np.uint8)
            if fmt == GRAY8_X2:
                pad[:, :2 * w] = owner.reshape(h, 2 * w)
                view = np.lib.stride_tricks.as_strided(pad, (h, w, 2), (pad.strides[0], 2, 1))[..., 1]
                want_pad = gb
            else:
                pad[:, :w * BPP[fmt]] = a.reshape(h, -1)
                view = np.lib.stride_tricks.as_strided(pad, a.shape, (pad.strides[0], BPP[fmt], 1))
                want_pad = ga
            ctx.batch_upload_image(2, view)
            # device memory
            raw = torch.from_numpy(owner if fmt == GRAY8_X2 else b).to(dev)
            torch.cuda.synchronize()
            ctx.batch_upload_image_dev(3, raw.data_ptr() + (1 if fmt == GRAY8_X2 else 0), w * BPP[fmt])
            ctx.batch_sync()
            for idx, want in ((0, ga), (1, gb), (2, want_pad), (3, gb)):
                got = ctx.batch_get_pyramid_level(idx, 0)
                assert np.array_equal(got, want), (NAMES[fmt], (w, h), idx, int((got != want).sum()))
        finally:
            ctx.close()


# ------------------------------------------------------------------ synchronous calls
def _drop_in_run(ctx, frames, pts, P_l, P_r):
    """four images, then the kept pair, circular matching (with and without images), detection on an image of its own and on
    the kept pair's left image"""
    (l0, r0), (l1, r1), (l2, r2) = frames
    out = {}
    out["track4"] = ctx.track_frame(l0, r0, l1, r1, pts, P_l, P_r)
    out["track_kept"] = ctx.track_frame(None, None, l2, r2, pts, P_l, P_r, tvec=out["track4"]["tvec"])
    out["bucket_kept"] = ctx.detect_bucket(None, np.zeros((0, 2), np.float32), np.zeros(0, np.int32))
    out["circ4"] = ctx.circular_match(l0, r0, l1, r1, pts, apply_consistency=True)
    out["circ_kept"] = ctx.circular_match(None, None, l2, r2, pts)
    out["bucket_own"] = ctx.detect_bucket(l0, pts[:40], np.arange(40, dtype=np.int32), features_per_bucket=2)
    out["fast_own"] = ctx.fast_detect(r1)
    return out


@fmt_param
def test_drop_in_calls_equal_the_gray_calls(volib, small4, small_world, fmt):
    from visual_odom_amd import synth
    L, R = small4
    h, w = L[0].shape
    P_l, P_r = small_world.proj_matrices()
    enc = [encode_pair(L[k], R[k], fmt, 10 * k) for k in range(3)]
    pts = synth.select_keypoints(enc[0][2], bucket=16, per_bucket=2)
    res = {}
    for name, f, frames in (("fmt", fmt, [(e[0], e[1]) for e in enc]), ("gray", GRAY8, [(e[2], e[3]) for e in enc])):
        ctx = volib.Context(0, w, h, 4096, 1)
        try:
            ctx.set_params(input_format=f)
            pinned_schedule(ctx)
            res[name] = _drop_in_run(ctx, frames, pts, P_l, P_r)
        finally:
            ctx.close()
    assert len(res["gray"]["track4"]["l1"]) > 50 and len(res["gray"]["fast_own"]) > 100   # (the comparison is not empty)
    same(res["fmt"], res["gray"], NAMES[fmt])


@pytest.mark.parametrize("fmt,which", [(BGR8, "vga"), (GRAY8_X2, "vga"), (RGBA8, "kitti"), (GRAY8_X2, "kitti")],
                         ids=["bgr8-640x480", "gray8_x2-640x480", "rgba8-1241x376", "gray8_x2-1241x376"])
def test_track_frame_at_sensor_and_kitti_size(volib, vga_pair, kitti_seq, kitti_world, fmt, which):
    from visual_odom_amd import synth
    if which == "vga":
        L, R, (P_l, P_r) = vga_pair
    else:
        L, R, (P_l, P_r) = kitti_seq["L"], kitti_seq["R"], kitti_world.proj_matrices()
    h, w = L[0].shape
    enc = [encode_pair(L[k], R[k], fmt, 3 + k) for k in range(2)]
    pts = synth.select_keypoints(enc[0][2], bucket=h // 10, per_bucket=3)
    res = {}
    for name, f, i, j in (("fmt", fmt, 0, 1), ("gray", GRAY8, 2, 3)):
        ctx = volib.Context(0, w, h, 4096, 1)
        try:
            ctx.set_params(input_format=f)
            pinned_schedule(ctx)
            res[name] = ctx.track_frame(enc[0][i], enc[0][j], enc[1][i], enc[1][j], pts, P_l, P_r)
        finally:
            ctx.close()
    assert len(res["gray"]["l1"]) > 100
    same(res["fmt"], res["gray"], (NAMES[fmt], which))


# ------------------------------------------------------------------ lock-step loop
def _loop(volib, S, w, h, P_l, P_r, fmt, kind, pair_of, n_steps, split_planes=False):
    """n_steps steps of S sequences through vo_seq_push_pairs(kind); pair_of(s, k) -> encode_pair's tuple.  split_planes (X2):
    the right plane comes from ANOTHER frame buffer than the left one, so the pair is not one interleaved buffer"""
    import torch
    dev = torch.device("cuda", 0)
    ctx = volib.Context(0, w, h, 2048, S)
    try:
        ctx.set_params(input_format=fmt)
        pinned_schedule(ctx)
        ctx.batch_set_detect_params(features_per_bucket=2)
        ctx.seq_configure(S, w, h, ring=3, max_steps=16)
        ctx.batch_set_projection(P_l, P_r)
        keep = []
        stride = w * BPP[fmt]
        for k in range(n_steps):
            lp, rp, own = [], [], []
            for s in range(S):
                a, b, ga, gb, owner = pair_of(s, k)
                if fmt == GRAY8:
                    srcs = [np.ascontiguousarray(ga), np.ascontiguousarray(gb)]
                elif fmt == GRAY8_X2 and not split_planes:
                    srcs = [owner]                                               # ONE buffer: left = buf, right = buf + 1
                elif fmt == GRAY8_X2:
                    srcs = [owner, np.ascontiguousarray(np.stack([gb, gb], axis=-1))]   # right plane = high bytes of another buffer
                else:
                    srcs = [a, b]
                base = []
                for src in srcs:
                    if kind == 0:
                        t = src
                        base.append(t.ctypes.data)
                    else:
                        t = torch.from_numpy(src).pin_memory() if kind == 1 else torch.from_numpy(src).to(dev)
                        base.append(t.data_ptr())
                    own.append(t)
                lp.append(base[0])
                rp.append(base[-1] + (1 if fmt == GRAY8_X2 else 0))
            if kind == 2:
                torch.cuda.synchronize()
            ctx.seq_push_pairs(ctx.seq_pair_table(range(S), lp, rp), stride, kind)
            keep.append(own)   # (page-locked / device sources stay alive until their step has run)
            ctx.seq_step()
        ctx.seq_sync()
        return [ctx.seq_get_trajectory(s) for s in range(S)], [ctx.seq_get_state(s) for s in range(S)]
    finally:
        ctx.close()


def _same_loop(got, base, what):
    (traj, state), (base_t, base_s) = got, base
    for s in range(len(base_t)):
        assert traj[s][0].tobytes() == base_t[s][0].tobytes() and np.array_equal(traj[s][1], base_t[s][1]), (what, s, "trajectory")
        for i in range(3):
            assert state[s][i].shape == base_s[s][i].shape and state[s][i].tobytes() == base_s[s][i].tobytes(), (what, s, "state", i)


@pytest.mark.parametrize("S", [2, 40])
def test_lockstep_loop_equals_the_gray_loop(volib, small_world, S):
    """6 steps; kinds 0 (pageable; at S = 40 the all-pageable one-transfer path), 1 (page-locked, torch pin_memory) and 2
    (device); every format; the interleaved format both as ONE buffer per pair (read once) and as two planes of different buffers"""
    n = 6
    L, R, _, _ = small_world.render_sequence(n + 3)
    h, w = L[0].shape
    P_l, P_r = small_world.proj_matrices()
    cache = {}
    for fmt in FORMATS:
        def pair_of(s, k, fmt=fmt):
            key = (fmt, k + s % 3)
            if key not in cache:   # sequence s is the same street, three phases
                cache[key] = encode_pair(L[k + s % 3], R[k + s % 3], fmt, 100 + k + s % 3)
            return cache[key]
        base = _loop(volib, S, w, h, P_l, P_r, GRAY8, 0, pair_of, n)   # the gray loop on numpy's conversion of the same arrays
        assert all(len(r) == n - 1 for r, _ in base[0]) and sum(int((i[:, 5] & 2 != 0).sum()) for _, i in base[0]) > S * (n - 1) // 2
        for kind in (0, 1, 2):
            _same_loop(_loop(volib, S, w, h, P_l, P_r, fmt, kind, pair_of, n), base, (NAMES[fmt], "kind", kind, "S", S))
        if fmt == GRAY8_X2 and S == 2:
            for kind in (0, 1):
                _same_loop(_loop(volib, S, w, h, P_l, P_r, fmt, kind, pair_of, n, split_planes=True), base, ("x2 split planes", kind))


# ------------------------------------------------------------------ the python frame loops
@pytest.mark.parametrize("fmt", [GRAY8_X2, RGB8], ids=["gray8_x2", "rgb8"])
def test_odometry_classes_take_the_format(volib, small_world, fmt):
    from visual_odom_amd import odometry
    n = 5
    L, R, _, _ = small_world.render_sequence(n)
    h, w = L[0].shape
    P_l, P_r = small_world.proj_matrices()
    enc = [encode_pair(L[k], R[k], fmt, 40 + k) for k in range(n)]
    logs, trajs, seq = {}, {}, {}
    for name, f, i, j in (("fmt", fmt, 0, 1), ("gray", GRAY8, 2, 3)):
        vo = odometry.StereoOdometry(P_l, P_r, max_w=w, max_h=h, input_format=f)
        try:
            pinned_schedule(vo.ctx)
            for e in enc:
                vo.process(e[i], e[j])
            logs[name], trajs[name] = vo.log, np.array(vo.trajectory)
        finally:
            vo.close()
        ms = odometry.MultiSequenceOdometry(P_l, P_r, 2, w, h, max_steps=8, input_format=f)
        try:
            for k in range(n):
                for s in range(2):
                    e = enc[(k + s) % n]
                    ms.push(s, e[i], e[j])
                ms.step()
            ms.sync()
            seq[name] = [(ms.trajectory(s), ms.log(s), ms.state(s)) for s in range(2)]
        finally:
            ms.close()
    assert len(logs["gray"]) == n - 1 and trajs["fmt"].tobytes() == trajs["gray"].tobytes()
    for a, b in zip(logs["fmt"], logs["gray"]):
        same({k: v for k, v in a.items()}, {k: v for k, v in b.items()}, "StereoOdometry record")
    for s in range(2):
        assert np.array(seq["fmt"][s][0]).tobytes() == np.array(seq["gray"][s][0]).tobytes()
        same(seq["fmt"][s][1], seq["gray"][s][1], "MultiSequenceOdometry log")
        for x, y in zip(seq["fmt"][s][2], seq["gray"][s][2]):
            assert x.tobytes() == y.tobytes()


# ------------------------------------------------------------------ errors, and the way back to gray
def test_bad_formats_and_short_strides_are_refused(volib, small4, small_world):
    import torch
    L, R = small4
    h, w = L[0].shape
    P_l, P_r = small_world.proj_matrices()
    lib = volib.load()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    ctx = volib.Context(0, w, h, 256, 2)
    try:
        for bad in (6, -1):
            with pytest.raises(volib.VoError) as e:
                ctx.set_params(input_format=bad)
            assert e.value.code == volib.VO_ERR_ARG
        assert ctx.get_params().input_format == GRAY8 and ctx.input_format == GRAY8
        pts = np.array([[100, 60], [200, 80]], np.float32)
        f32 = lambda *s: np.zeros(s, np.float32)   # noqa: E731
        i32 = lambda *s: np.zeros(s, np.int32)     # noqa: E731
        n_out, n_circ, n_inl, n_pts, n_ages = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        for fmt in [GRAY8] + FORMATS:
            ctx.set_params(input_format=fmt)
            bpp = BPP[fmt]
            img = np.zeros((h, w * bpp), np.uint8)
            short = w * bpp - 1
            dimg = torch.zeros((h, w * bpp), dtype=torch.uint8, device="cuda")
            o = [f32(8, 2) for _ in range(5)]
            rv, tv, Rm = np.zeros(3), np.zeros(3), np.zeros(9)
            for stride, want in ((short, volib.VO_ERR_ARG), ):
                assert lib.vo_track_frame(ctx.h, vp(img), vp(img), vp(img), vp(img), w, h, stride, vp(pts), 2, vp(P_l), vp(P_r), vp(o[0]),
                                          vp(o[1]), vp(o[2]), vp(o[3]), vp(f32(8, 3)), vp(i32(8)), C.byref(n_out), vp(i32(8)),
                                          C.byref(n_circ), vp(rv), vp(tv), vp(Rm), vp(i32(8)), C.byref(n_inl)) == want, (fmt, "track")
                assert lib.vo_circular_match(ctx.h, vp(img), vp(img), vp(img), vp(img), w, h, stride, vp(pts), 2, vp(o[0]), vp(o[1]),
                                             vp(o[2]), vp(o[3]), vp(o[4]), None, None, C.byref(n_out), 0) == want, (fmt, "circ")
                assert lib.vo_fast_detect(ctx.h, vp(img), w, h, stride, 20, 1, vp(f32(64, 2)), 64, C.byref(n_out)) == want, (fmt, "fast")
                assert lib.vo_detect_bucket(ctx.h, vp(img), w, h, stride, None, vp(f32(256, 2)), C.byref(n_pts), vp(i32(256)),
                                            C.byref(n_ages), 256) == want, (fmt, "bucket")
                ctx.batch_configure(4, w, h, 1)
                assert lib.vo_batch_upload_image(ctx.h, 0, vp(img), stride) == want, (fmt, "upload")
                assert lib.vo_batch_upload_image_dev(ctx.h, 0, C.c_void_p(dimg.data_ptr()), stride) == want, (fmt, "upload_dev")
                ctx.seq_configure(2, w, h, ring=3, max_steps=4)
                assert lib.vo_seq_push_pair(ctx.h, 0, vp(img), vp(img), stride, 0) == want, (fmt, "push")
                assert lib.vo_seq_push_pair_dev(ctx.h, 0, C.c_void_p(dimg.data_ptr()), C.c_void_p(dimg.data_ptr()), stride) == want, (fmt, "push_dev")
                ids = (C.c_int32 * 1)(0)
                ptrs = (C.c_void_p * 1)(img.ctypes.data)
                for kind in (0, 1, 2):
                    assert lib.vo_seq_push_pairs(ctx.h, 1, ids, ptrs, ptrs, stride, kind) == want, (fmt, "push_pairs", kind)
                for kind in (3, -1):
                    assert lib.vo_seq_push_pairs(ctx.h, 1, ids, ptrs, ptrs, w * bpp, kind) == want
            # the exact minimum is accepted
            ctx.batch_configure(4, w, h, 1)
            assert lib.vo_batch_upload_image(ctx.h, 0, vp(img), w * bpp) == volib.VO_OK, fmt
    finally:
        ctx.close()


def test_a_context_set_back_to_gray_behaves_as_before(volib, small4, small_world):
    from visual_odom_amd import synth
    L, R = small4
    h, w = L[0].shape
    P_l, P_r = small_world.proj_matrices()
    pts = synth.select_keypoints(L[0], bucket=16, per_bucket=2)
    ctx = volib.Context(0, w, h, 4096, 1)
    fresh = volib.Context(0, w, h, 4096, 1)
    try:
        pinned_schedule(ctx)
        pinned_schedule(fresh)
        ctx.set_params(input_format=BGRA8)
        a, b, _, _, _ = encode_pair(L[0], R[0], BGRA8, 1)
        c, d, _, _, _ = encode_pair(L[1], R[1], BGRA8, 2)
        ctx.track_frame(a, b, c, d, pts, P_l, P_r)
        ctx.set_params(input_format=GRAY8)
        with pytest.raises(volib.VoError) as e:   # the kept pair does not survive a change of format (a new configure)
            ctx.track_frame(None, None, L[2], R[2], pts, P_l, P_r)
        assert e.value.code == volib.VO_ERR_STATE
        got = ctx.track_frame(L[0], R[0], L[1], R[1], pts, P_l, P_r)
        want = fresh.track_frame(L[0], R[0], L[1], R[1], pts, P_l, P_r)
        same(got, want, "gray again")
        same(ctx.track_frame(None, None, L[2], R[2], pts, P_l, P_r, tvec=got["tvec"]),
             fresh.track_frame(None, None, L[2], R[2], pts, P_l, P_r, tvec=want["tvec"]), "gray again, kept pair")
    finally:
        ctx.close()
        fresh.close()
