"""Rectification at ingest on the MI355X (-m gpu): a context with maps (vo_params.rectify) fed RAW frames against the SAME calls
of a context without maps fed with images remapped on the host by the numpy restatement of the formula of include/vo_hip.h
(tests/rectify_cases.py: remap_ref).  Every comparison is bit for bit -- pixels of every pyramid level, every output array,
count, status, rvec / tvec, trajectory rows, info and state.  Left and right maps differ everywhere, so a swapped side fails.
Schedules are pinned in both contexts of a comparison (a schedule never changes a result; pinning only skips the probes' time).

Against a vacuous pass the comparator must keep at least 20 survivors and return VO_OK on every input.  The mild maps of the
tracking calls (rectify_cases.mild_maps: k1 = -0.05 / -0.045, rotations of 0.3 / -0.25 degrees, up to 9.4 pixels of displacement
at 480 x 160 and 16 at 640 x 480) were checked on the CPU with the oracle on the remapped images: small_world pairs (0, 1), (1, 2),
(2, 3): 523 / 526 / 491 of 596 points survive the circular match, 465 / 455 / 390 the consistency filter, solvePnPRansac finds a
model each time, FAST finds 1208 / 1179 / 1232 corners; the 640 x 480 pair: 255 of 420, then 222, a model, 2590 corners."""
import ctypes as C

import numpy as np
import pytest

from rectify_cases import HEIGHTS, MAP_KINDS, WIDTHS, make_image, make_maps, mild_maps, remap_ref

pytestmark = pytest.mark.gpu

GRAY8, GRAY8_X2, BGR8 = 0, 1, 2
FMT_NAMES = {GRAY8: "gray8", GRAY8_X2: "gray8_x2", BGR8: "bgr8"}


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


def to_gray_bgr(px):
    p = px.astype(np.int64)
    return ((p[..., 0] * 1868 + p[..., 1] * 9617 + p[..., 2] * 4899 + 8192) >> 14).astype(np.uint8)


def encode_pair(left, right, fmt, seed):
    """a RAW stereo pair as a context of format `fmt` takes it -> (left array, right array, left gray, right gray, owner)"""
    if fmt == GRAY8:
        return left, right, left, right, None
    if fmt == GRAY8_X2:   # ONE buffer of 16-bit words: left = low byte, right = high byte
        frame = np.ascontiguousarray(np.stack([left, right], axis=-1))
        return frame[..., 0], frame[..., 1], frame[..., 0].copy(), frame[..., 1].copy(), frame
    rng = np.random.default_rng(seed)
    out = []
    for g in (left.astype(np.float64), right.astype(np.float64)):   # channels that differ from each other
        out.append(np.ascontiguousarray(np.stack([np.clip(g * 0.85 + 40 + rng.integers(-6, 7, g.shape), 0, 255),
                                                  np.clip(g * 1.05 - 9 + rng.integers(-4, 5, g.shape), 0, 255),
                                                  np.clip(g * 0.70 + 25 + rng.integers(-9, 10, g.shape), 0, 255)], axis=-1).astype(np.uint8)))
    return out[0], out[1], to_gray_bgr(out[0]), to_gray_bgr(out[1]), None


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


def all_levels(ctx, idx):
    out = []
    for level in range(5):
        w, h = C.c_int(0), C.c_int(0)
        if ctx.lib.vo_batch_get_pyramid_level(ctx.h, idx, level, None, C.byref(w), C.byref(h)) != 0:
            break
        out.append(ctx.batch_get_pyramid_level(idx, level))
    return out


# ------------------------------------------------------------------ pixels: level 0 is numpy's remap, the pyramid follows
@pytest.mark.parametrize("kind", MAP_KINDS)
def test_pixels_and_pyramids(volib, kind):
    """every shape of the CPU tier (configure accepts all of them: 32 x 32 is its minimum), host and device sources, a padded
    host buffer, both sides; all pyramid levels are compared, so the stage downstream sees the same image"""
    import torch
    dev = torch.device("cuda", 0)
    ctx = volib.Context(0, max(WIDTHS), max(HEIGHTS), 64, 1)
    ref = volib.Context(0, max(WIDTHS), max(HEIGHTS), 64, 1)
    try:
        for w in WIDTHS:
            for h in HEIGHTS:
                rng = np.random.default_rng(17 * w + h)
                maps = [make_maps(kind, w, h, side) for side in (0, 1)]
                raws = [make_image(rng, w, h) for _ in range(4)]
                ctx.set_params(rectify=maps)
                ctx.batch_configure(4, w, h, 1)
                ref.batch_configure(4, w, h, 1)
                ctx.batch_upload_image(0, raws[0])                      # left, host
                pad = np.full((h, w + 19), 0xEE, np.uint8)
                pad[:, :w] = raws[1]
                ctx.batch_upload_image(1, pad[:, :w])                   # right, host, a padded buffer
                t2, t3 = torch.from_numpy(raws[2]).to(dev), torch.from_numpy(pad).to(dev)
                t3[:, :w] = torch.from_numpy(raws[3]).to(dev)
                torch.cuda.synchronize()
                ctx.batch_upload_image_dev(2, t2.data_ptr(), w)         # left, device
                ctx.batch_upload_image_dev(3, t3.data_ptr(), w + 19)    # right, device, padded
                want = [remap_ref(raws[i], *maps[i & 1]) for i in range(4)]
                for i in range(4):
                    ref.batch_upload_image(i, want[i])
                for c in (ctx, ref):
                    c.batch_run(volib.STAGE_PYRAMID)
                    c.batch_sync()
                for i in range(4):
                    got, exp = all_levels(ctx, i), all_levels(ref, i)
                    assert np.array_equal(got[0], want[i]), (kind, (w, h), i, int((got[0] != want[i]).sum()))
                    assert len(got) == len(exp) >= 1
                    for lv, (g, e) in enumerate(zip(got, exp)):
                        assert np.array_equal(g, e), (kind, (w, h), i, "level", lv)
                if kind == "identity":
                    assert np.array_equal(want[0], raws[0]) and not np.array_equal(want[1], raws[1])
    finally:
        ctx.close()
        ref.close()


# ------------------------------------------------------------------ synchronous calls
def _drop_in_run(ctx, frames, pts, P_l, P_r):
    (l0, r0), (l1, r1), (l2, r2) = frames
    out = {}
    out["track4"] = ctx.track_frame(l0, r0, l1, r1, pts, P_l, P_r)
    out["track_kept"] = ctx.track_frame(None, None, l2, r2, pts, P_l, P_r, tvec=out["track4"]["tvec"])
    out["bucket_kept"] = ctx.detect_bucket(None, np.zeros((0, 2), np.float32), np.zeros(0, np.int32))
    out["circ4"] = ctx.circular_match(l0, r0, l1, r1, pts, apply_consistency=True)
    out["circ_kept"] = ctx.circular_match(None, None, l2, r2, pts)
    out["bucket_own"] = ctx.detect_bucket(l0, pts[:40], np.arange(40, dtype=np.int32), features_per_bucket=2)
    return out


@pytest.mark.parametrize("fmt", [GRAY8, BGR8, GRAY8_X2], ids=lambda f: FMT_NAMES[f])
def test_drop_in_calls_equal_the_calls_on_remapped_images(volib, small4, small_world, fmt):
    """vo_track_frame with four images and on the kept pair, vo_circular_match, vo_detect_bucket (kept pair and an image of its
    own: left maps); with a colour format and with ONE interleaved buffer the conversion comes first"""
    from visual_odom_amd import synth
    L, R = small4
    h, w = L[0].shape
    P_l, P_r = small_world.proj_matrices()
    maps = mild_maps(P_l, w, h)
    enc = [encode_pair(L[k], R[k], fmt, 10 * k) for k in range(3)]
    rect = [(remap_ref(e[2], *maps[0]), remap_ref(e[3], *maps[1])) for e in enc]
    pts = synth.select_keypoints(rect[0][0], bucket=16, per_bucket=2)
    res = {}
    for name, frames in (("rect", [(e[0], e[1]) for e in enc]), ("plain", rect)):
        ctx = volib.Context(0, w, h, 4096, 1)
        try:
            if name == "rect":
                ctx.set_params(input_format=fmt, rectify=maps)
                p = ctx.get_params()
                assert (p.rectify, p.rect_w, p.rect_h, p.rect_map_stride) == (1, w, h, 4 * w)
            pinned_schedule(ctx)
            res[name] = _drop_in_run(ctx, frames, pts, P_l, P_r)
            if name == "rect":   # vo_fast_detect is cv::FAST's counterpart: the RAW image, never rectified
                res["fast_raw"] = ctx.fast_detect(enc[1][1])
            else:
                res["fast_want"] = ctx.fast_detect(enc[1][3])
        finally:
            ctx.close()
    base = res["plain"]
    for k in ("track4", "track_kept"):
        assert base[k]["rc"] == volib.VO_OK and len(base[k]["l1"]) >= 20 and len(base[k]["inliers"]) >= 20, k
    assert base["circ4"]["n_out"] >= 20 and base["circ_kept"]["n_out"] >= 20
    assert len(base["bucket_kept"][0]) >= 20 and len(base["bucket_own"][0]) >= 20 and len(res["fast_want"]) >= 100
    same(res["rect"], base, FMT_NAMES[fmt])
    same(res["fast_raw"], res["fast_want"], "fast_detect reads the raw image")


def test_track_frame_at_sensor_size(volib, vga_pair):
    from visual_odom_amd import synth
    L, R, (P_l, P_r) = vga_pair
    h, w = L[0].shape
    maps = mild_maps(P_l, w, h)
    rect = [(remap_ref(L[k], *maps[0]), remap_ref(R[k], *maps[1])) for k in range(2)]
    pts = synth.select_keypoints(rect[0][0], bucket=h // 10, per_bucket=3)
    res = {}
    for name in ("rect", "plain"):
        ctx = volib.Context(0, w, h, 4096, 1)
        try:
            if name == "rect":
                ctx.set_params(rectify=maps)
            pinned_schedule(ctx)
            f = [(L[0], R[0]), (L[1], R[1])] if name == "rect" else rect
            res[name] = ctx.track_frame(f[0][0], f[0][1], f[1][0], f[1][1], pts, P_l, P_r)
        finally:
            ctx.close()
    assert res["plain"]["rc"] == volib.VO_OK and len(res["plain"]["l1"]) >= 20
    same(res["rect"], res["plain"], "640 x 480")


def test_batch_run_of_three_frames(volib, small4, small_world):
    """vo_batch_run(VO_STAGE_ALL | VO_STAGE_DETECT) over three frames of an eight-image table: even index = left, odd = right"""
    L, R = small4
    h, w = L[0].shape
    P_l, P_r = small_world.proj_matrices()
    maps = mild_maps(P_l, w, h)
    res = {}
    for name in ("rect", "plain"):
        ctx = volib.Context(0, w, h, 2048, 3)
        try:
            if name == "rect":
                ctx.set_params(rectify=maps)
            pinned_schedule(ctx)
            ctx.batch_configure(8, w, h, 3)
            for k in range(4):
                for side, img in enumerate((L[k], R[k])):
                    ctx.batch_upload_image(2 * k + side, img if name == "rect" else remap_ref(img, *maps[side]))
            ctx.batch_set_quads([[2 * k, 2 * k + 1, 2 * k + 2, 2 * k + 3] for k in range(3)])
            ctx.batch_set_projection(P_l, P_r)
            ctx.batch_set_detect_params(features_per_bucket=2)
            for f in range(3):
                ctx.batch_set_features(f, np.zeros((0, 2), np.float32), np.zeros(0, np.int32))
            ctx.batch_run(volib.STAGE_ALL | volib.STAGE_DETECT)
            ctx.batch_sync()
            res[name] = [(ctx.batch_get_features(f), ctx.batch_get_filtered(f), ctx.batch_get_pose(f)) for f in range(3)]
        finally:
            ctx.close()
    for feats, filt, pose in res["plain"]:
        assert len(feats[0]) >= 20 and len(filt["l1"]) >= 20 and pose["status"] == 1
    same(res["rect"], res["plain"], "batch")


# ------------------------------------------------------------------ lock-step loop
def _loop(volib, S, w, h, P_l, P_r, maps, kind, pair_of, n_steps, ring):
    import torch
    dev = torch.device("cuda", 0)
    ctx = volib.Context(0, w, h, 2048, S)
    try:
        if maps is not None:
            ctx.set_params(rectify=maps)
        pinned_schedule(ctx)
        ctx.batch_set_detect_params(features_per_bucket=2)
        ctx.seq_configure(S, w, h, ring=ring, max_steps=16)
        ctx.batch_set_projection(P_l, P_r)
        keep = []
        for k in range(n_steps):
            lp, rp, own = [], [], []
            for s in range(S):
                for src, ptrs in zip(pair_of(s, k), (lp, rp)):
                    if kind == 0:
                        t = src
                        ptrs.append(t.ctypes.data)
                    else:
                        t = torch.from_numpy(src).pin_memory() if kind == 1 else torch.from_numpy(src).to(dev)
                        ptrs.append(t.data_ptr())
                    own.append(t)
            if kind == 2:
                torch.cuda.synchronize()
            ctx.seq_push_pairs(ctx.seq_pair_table(range(S), lp, rp), w, kind)
            keep.append(own)   # (page-locked / device sources stay alive until their step has run)
            ctx.seq_step()
        ctx.seq_sync()
        return [ctx.seq_get_trajectory(s) for s in range(S)], [ctx.seq_get_state(s) for s in range(S)]
    finally:
        ctx.close()


@pytest.mark.parametrize("S,ring", [(3, 2), (3, 3), (32, 3)], ids=["S3-ring2", "S3-ring3", "S32-one-transfer"])
def test_lockstep_loop_equals_the_loop_on_remapped_images(volib, small_world, S, ring):
    """4 steps; pairs pageable (at S = 32 the all-pageable one-transfer path), page-locked and device: trajectory rows, info and
    vo_seq_get_state are those of a loop without maps on the remapped pairs"""
    n = 4
    L, R, _, _ = small_world.render_sequence(n + 2)
    h, w = L[0].shape
    P_l, P_r = small_world.proj_matrices()
    maps = mild_maps(P_l, w, h)
    rect = [(remap_ref(L[k], *maps[0]), remap_ref(R[k], *maps[1])) for k in range(n + 2)]
    raw_of = lambda s, k: (np.ascontiguousarray(L[k + s % 3]), np.ascontiguousarray(R[k + s % 3]))   # noqa: E731  (three phases of one street)
    rect_of = lambda s, k: rect[k + s % 3]                  # noqa: E731
    base = _loop(volib, S, w, h, P_l, P_r, None, 0, rect_of, n, ring)
    for rows, info in base[0]:
        assert len(rows) == n - 1 and np.all(info[:, 2] >= 20) and np.all(info[:, 4] == 1), info   # n_tracked, pnp_status
    for kind in (0, 1, 2):
        traj, state = _loop(volib, S, w, h, P_l, P_r, maps, kind, raw_of, n, ring)
        for s in range(S):
            assert traj[s][0].tobytes() == base[0][s][0].tobytes() and np.array_equal(traj[s][1], base[0][s][1]), (kind, s, "trajectory")
            for i in range(3):
                assert state[s][i].shape == base[1][s][i].shape and state[s][i].tobytes() == base[1][s][i].tobytes(), (kind, s, "state", i)


def test_odometry_classes_take_the_maps(volib, small_world):
    from visual_odom_amd import odometry
    n = 4
    L, R, _, _ = small_world.render_sequence(n)
    h, w = L[0].shape
    P_l, P_r = small_world.proj_matrices()
    maps = mild_maps(P_l, w, h)
    out = {}
    for name in ("rect", "plain"):
        frames = [(L[k], R[k]) if name == "rect" else (remap_ref(L[k], *maps[0]), remap_ref(R[k], *maps[1])) for k in range(n)]
        vo = odometry.StereoOdometry(P_l, P_r, max_w=w, max_h=h, rectify=maps if name == "rect" else None)
        try:
            pinned_schedule(vo.ctx)
            for l, r in frames:
                vo.process(l, r)
            out[name] = [np.array(vo.trajectory), vo.log]
        finally:
            vo.close()
        ms = odometry.MultiSequenceOdometry(P_l, P_r, 2, w, h, max_steps=8, rectify=maps if name == "rect" else None)
        try:
            for k in range(n):
                for s in range(2):
                    ms.push(s, *frames[(k + s) % n])
                ms.step()
            ms.sync()
            out[name] += [[(np.array(ms.trajectory(s)), ms.log(s)) for s in range(2)]]
        finally:
            ms.close()
    assert len(out["plain"][1]) == n - 1
    same(out["rect"], out["plain"], "python frame loops")


# ------------------------------------------------------------------ errors, and the way back
def test_errors_and_the_way_back_to_a_plain_context(volib, small4, small_world):
    from visual_odom_amd import synth
    L, R = small4
    h, w = L[0].shape
    P_l, P_r = small_world.proj_matrices()
    maps = mild_maps(P_l, w, h)
    lib = volib.load()
    pts = synth.select_keypoints(L[0], bucket=16, per_bucket=2)
    ctx = volib.Context(0, 1200, h, 4096, 2)
    fresh = volib.Context(0, 1200, h, 4096, 2)

    def refused(code, p):
        assert lib.vo_set_params(ctx.h, C.byref(p)) == code
        assert len(lib.vo_last_error(ctx.h)) > 10
        assert ctx.get_params().rectify == 0, "a refused vo_set_params changes nothing"

    try:
        pinned_schedule(ctx)
        pinned_schedule(fresh)
        # a NULL map, a short stride, a size beyond vo_create's, an over-range displacement
        p = ctx.get_params()
        keep = p.set_rectify_maps(maps)
        p.rect_map_y_right = None
        refused(volib.VO_ERR_ARG, p)
        p = ctx.get_params()
        keep = p.set_rectify_maps(maps)
        p.rect_map_stride = 4 * w - 4
        refused(volib.VO_ERR_ARG, p)
        p = ctx.get_params()
        tall = tuple((np.zeros((h + 1, w), np.float32), np.zeros((h + 1, w), np.float32)) for _ in range(2))
        keep = p.set_rectify_maps(tall)
        refused(volib.VO_ERR_ARG, p)
        wide = [list(make_maps("identity", 1200, h, s)) for s in (0, 1)]
        wide[1][0][7, 1190] = 100.0   # 1090 pixels from its own pixel, taps inside the image
        p = ctx.get_params()
        keep = p.set_rectify_maps(wide)
        refused(volib.VO_ERR_ARG, p)
        wide[1][0][7, 1190] = -50.0   # as far, but wholly outside: fine
        ctx.set_params(rectify=wide)
        assert ctx.get_params().rect_w == 1200
        # another size than the maps': configure and the synchronous calls
        ctx.set_params(rectify=maps)
        with pytest.raises(volib.VoError) as e:
            ctx.batch_configure(4, w + 1, h, 1)
        assert e.value.code == volib.VO_ERR_ARG and "rect_w" in str(e.value)
        with pytest.raises(volib.VoError) as e:
            ctx.track_frame(L[0][:, :w - 8], R[0][:, :w - 8], L[1][:, :w - 8], R[1][:, :w - 8], pts[:10], P_l, P_r)
        assert e.value.code == volib.VO_ERR_ARG
        with pytest.raises(volib.VoError) as e:
            ctx.seq_configure(2, w, h - 1, ring=2, max_steps=4)
        assert e.value.code == volib.VO_ERR_ARG
        # inside a running loop the maps cannot change
        ctx.seq_configure(2, w, h, ring=2, max_steps=4)
        ctx.batch_set_projection(P_l, P_r)
        ctx.seq_push_pair(0, L[0], R[0])
        ctx.seq_step()
        other = tuple((mx.copy(), my.copy()) for mx, my in maps)   # (other buffers: new maps as far as the library can tell)
        for new in (None, other):
            with pytest.raises(volib.VoError) as e:
                ctx.set_params(rectify=new)
            assert e.value.code == volib.VO_ERR_STATE and len(str(e.value)) > 30
        ctx.seq_sync()
        ctx.batch_configure(4, w, h, 1)   # leaves the loop
        # the maps work, and the caller's arrays are free after vo_set_params
        scratch = tuple((mx.copy(), my.copy()) for mx, my in maps)
        p = ctx.get_params()
        keep = p.set_rectify_maps(scratch)
        assert lib.vo_set_params(ctx.h, C.byref(p)) == volib.VO_OK
        for a in keep:
            a[:] = np.nan
        del keep, scratch
        # get / modify / set with the rectification fields untouched: "the maps you have" -- the dangling pointers are not read
        ctx.set_params(lk_max_count=29)
        ctx.set_params(lk_max_count=30)
        p = ctx.get_params()
        assert p.rectify == 1 and p.rect_w == w and bool(p.rect_map_x_left)
        got = ctx.track_frame(L[0], R[0], L[1], R[1], pts, P_l, P_r)
        want = fresh.track_frame(remap_ref(L[0], *maps[0]), remap_ref(R[0], *maps[1]), remap_ref(L[1], *maps[0]), remap_ref(R[1], *maps[1]),
                                 pts, P_l, P_r)
        assert len(want["l1"]) >= 20
        same(got, want, "maps freed after vo_set_params")
        # off again: bit-identical to a fresh context
        ctx.set_params(rectify=None)
        p = ctx.get_params()
        assert p.rectify == 0 and not bool(p.rect_map_x_left)
        with pytest.raises(volib.VoError) as e:   # (vo_set_params drops the kept pair, as it always did)
            ctx.track_frame(None, None, L[2], R[2], pts, P_l, P_r)
        assert e.value.code == volib.VO_ERR_STATE
        got = ctx.track_frame(L[0], R[0], L[1], R[1], pts, P_l, P_r)
        want = fresh.track_frame(L[0], R[0], L[1], R[1], pts, P_l, P_r)
        same(got, want, "plain again")
        same(ctx.track_frame(None, None, L[2], R[2], pts, P_l, P_r, tvec=got["tvec"]),
             fresh.track_frame(None, None, L[2], R[2], pts, P_l, P_r, tvec=want["tvec"]), "plain again, kept pair")
        ctx.batch_configure(4, w + 1, h, 1)   # any size again
    finally:
        ctx.close()
        fresh.close()
