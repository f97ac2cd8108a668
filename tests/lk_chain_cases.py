"""Inputs and expected results of the LK kernel tests at the smallest shapes where the search tile's fill and clamping matter
(test_lk_tile_emulation.py on the CPU emulator, test_gpu_lk_tile.py on the MI355X), and the emulator harness of the batched chain
(tests/host_check/chain_emu.cpp).

Shapes: 131 x 97 (three levels; 33 x 25 at the top) and 169 x 169, the smallest image with a level 3 (22 x 22: the 48 x 40 tile is
wider and taller than the level, its origin clamped on both axes).  Images: test_oracle_images.smooth_image at four shifts of up
to +-12 pixels, so tiles are refilled within a level.  Points: a grid that holds 0, 0.5 and w - 1.5, w - 1 on both axes
-- positions within a pixel of every border -- in a fixed shuffled order, so that every prefix holds border points.  Batches of 1,
3 and 9 frames (parts of a frame's list over 8 and 4 XCDs; a group of 8 frames and a partial one), frame f with its own quad (the
four images rotated by f) and its own number of points.  The checker's answers are computed once per session and never modified."""
import ctypes as C

import numpy as np

import emu_build
import flow_cases as fc
import flow_flags_cases as gc
import flow_win_cases as wc
from conftest import vp
from test_oracle_images import smooth_image

SHAPES = ((131, 97), (169, 169))          # (w, h)
SHIFTS = ((0.0, 0.0), (11.6, -3.4), (-7.3, 12.0), (-12.0, -9.7))
BATCHES = (1, 3, 9)
WINDOWS = (5, 13, 19, 21)
ALL_WINDOWS = tuple(range(5, 22, 2))      # lk_flow_flags_kernel<W> is one binary per window: the flag tests run every one
_CACHE = {}


def images(shape):
    key = ("images", shape)
    if key not in _CACHE:
        w, h = shape
        _CACHE[key] = [smooth_image(w, h, dx, dy, seed=w) for dx, dy in SHIFTS]
        for im in _CACHE[key]:
            im.setflags(write=False)
    return _CACHE[key]


def points(shape):
    key = ("points", shape)
    if key not in _CACHE:
        w, h = shape
        axis = lambda n: np.array([0, 0.5, n - 1.5, n - 1.0] + list(np.arange(8.25, n - 3, 29.5)), np.float32)
        pts = np.stack(np.meshgrid(axis(w), axis(h)), -1).reshape(-1, 2).astype(np.float32)
        pts = np.ascontiguousarray(pts[np.random.default_rng(w).permutation(len(pts))])
        pts.setflags(write=False)
        _CACHE[key] = pts
    return _CACHE[key]


def quads(n_frames):
    return np.array([np.roll([0, 1, 2, 3], -f) for f in range(n_frames)], np.int32)


def counts(n_frames, n):
    """points of frame f: all of them in frame 0, 23 fewer per frame, at least 3"""
    return np.array([max(3, n - 23 * f) for f in range(n_frames)], np.int32)


def oracle_chain(orc, shape, rot):
    """the checker's four hops (trk [4, n, 2], status [4, n]) over the images rotated by rot, every point"""
    key = ("chain", shape, rot % 4)
    if key not in _CACHE:
        im = images(shape)
        l0, r0, l1, r1 = (im[i] for i in quads(4)[rot % 4])
        e = wc.depth(shape[0], shape[1], 3)
        trk, st, p = [], [], points(shape)
        for a, b in ((l0, r0), (r0, r1), (r1, l1), (l1, l0)):
            p, s, _ = orc.calc_optical_flow_pyr_lk(a, b, p, max_level=e)
            trk.append(p)
            st.append(s)
        _CACHE[key] = fc.freeze((np.stack(trk), np.stack(st)))
    return _CACHE[key]


def chain_premises(shape, want):
    """the checker's side: the depth, tracked and lost points, a refilled tile (a move beyond what one tile holds around the start)"""
    trk, st = want
    p = points(shape)
    assert wc.depth(shape[0], shape[1], 3) == (2 if shape == (131, 97) else 3)
    assert (st[0] == 1).sum() >= len(p) // 2 and (st == 0).sum() >= 1
    move = np.abs(trk[0] - p)[st[0] == 1].max(0)
    assert move[0] > 9 or move[1] > 7, move          # 48 - 22 - 12 - 3 columns, 40 - 22 - 9 rows of slack beside a centred window


def flow_case(shape, win, orc):
    """images 0 -> 1 of the shape, window win: the dict tests/flow_emu.py and the device calls take, want = the checker's answer"""
    key = ("flow", shape, win)
    if key not in _CACHE:
        im, e = images(shape), wc.depth(shape[0], shape[1], 3)
        want = fc.freeze(orc.calc_optical_flow_pyr_lk(im[0], im[1], points(shape), win=win, max_level=e))
        _CACHE[key] = dict(prev=im[0], next=im[1], pts=points(shape), win=win, lk_max_level=3, max_level=e, want=want)
    return _CACHE[key]


def guess_case(shape, win, orc):
    """the same pair started at prev + uniform(-6, 6): want = the checker started there (flow_flags_cases.driver)"""
    key = ("guess", shape, win)
    if key not in _CACHE:
        c = dict(flow_case(shape, win, orc))
        c["guess"] = (c["pts"] + np.random.default_rng(7).uniform(-6, 6, c["pts"].shape)).astype(np.float32)
        c["plain"] = c["want"]
        c["want"] = fc.freeze(gc.driver(c["prev"], c["next"], c["pts"], c["guess"], win=win, max_level=c["max_level"]))
        assert (fc.bits(c["want"][0]) != fc.bits(c["plain"][0])).any(1).sum() >= len(c["pts"]) // 2, "the start matters"
        _CACHE[key] = c
    return _CACHE[key]


def eig_set(shape, win, orc):
    """flow_flags_cases.eig_set's record for image 0 of the shape and its points (no table of counts: the floors are asserted)"""
    key = ("eig", shape, win)
    if key not in _CACHE:
        img, pts = images(shape)[0], points(shape)
        adm = gc.admissible(img, pts, win)
        ver = orc.calc_optical_flow_pyr_lk(img, img, pts, win=win, max_level=0, min_eig=-1.0)[1] == 1
        st3 = orc.calc_optical_flow_pyr_lk(img, img, pts, win=win, max_level=0, min_eig=1e-3)[1] == 1
        assert adm.all() and not (ver & ~adm).any() and ver.sum() >= len(pts) // 2
        _CACHE[key] = dict(img=img, pts=pts, win=win, adm=adm, verifiable=ver, below=ver & ~st3,
                           want_no_err=fc.freeze(gc.plain_no_err(orc, img, img, pts, win=win, max_level=0)))
    return _CACHE[key]


def flag_cases(shape, win, orc):
    """(guess case, eig record, the pair of the eig record as a flow case) of one window, with the test's premise: the checker
    started at the guess tracks at least 15 points and loses at least 15"""
    g, s = guess_case(shape, win, orc), eig_set(shape, win, orc)
    assert (g["want"][1] == 1).sum() >= 15 and (g["want"][1] == 0).sum() >= 15, (shape, win)
    return g, s, dict(prev=s["img"], next=s["img"], pts=s["pts"], win=win, lk_max_level=0)


# ---- the batched chain on the CPU emulator -----------------------------------------------------------------------------------
def emu_lib():
    """libchain_emu.so, built WITHOUT sanitizer flags whatever the environment says (nothing instrumented is loaded into python)"""
    lib = emu_build.shared("chain_emu")
    lib.ce_chain.restype = C.c_int
    return lib


def _inputs(shape, n_frames):
    w, h = shape
    p = points(shape)
    n = len(p)
    return np.ascontiguousarray(np.stack(images(shape))), quads(n_frames), counts(n_frames, n), np.ascontiguousarray(np.broadcast_to(p, (n_frames, n, 2))), n


def emu_chain(shape, n_frames, full_chain=1, split=0):
    """(trk [F, 4, n, 2], status [F, 4, n], counts [F]) of the emulated launch"""
    w, h = shape
    imgs, q, cnt, pts, n = _inputs(shape, n_frames)
    trk, st = np.zeros((n_frames, 4, n, 2), np.float32), np.zeros((n_frames, 4, n), np.uint8)
    levels = emu_lib().ce_chain(vp(imgs), 4, w, h, 3, vp(q), n_frames, vp(pts), vp(cnt), n, full_chain, split, vp(trk), vp(st))
    assert levels == wc.depth(w, h, 3) + 1
    return trk, st, cnt


def emu_chain_standalone(tmp_path, shape, n_frames, full_chain=1, split=0):
    """the same launch through the stand-alone ASan + UBSan program, run as a child: no report, exit status 0"""
    exe = emu_build.sanitized_program("chain_emu", "CHAIN_EMU_MAIN")
    w, h = shape
    imgs, q, cnt, pts, n = _inputs(shape, n_frames)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([w, h, 3, 4, n_frames, n, full_chain, split], np.int32).tobytes())
        f.write(imgs.tobytes() + q.tobytes() + cnt.tobytes() + pts.tobytes())
    emu_build.run_clean(exe, [fin, fout], 900)
    raw = np.fromfile(fout, np.uint8)
    k = n_frames * 4 * n
    return raw[:8 * k].view(np.float32).reshape(n_frames, 4, n, 2), raw[8 * k:9 * k].reshape(n_frames, 4, n), cnt


def assert_chain(orc, shape, got, what=""):
    """every frame's tracked rows against the checker's chain over its quad, positions and status bit for bit"""
    trk, st, cnt = got
    for f, c in enumerate(cnt):
        wt, ws = oracle_chain(orc, shape, f)
        assert np.array_equal(st[f][:, :c], ws[:, :c]), (what, shape, f, "status", np.argwhere(st[f][:, :c] != ws[:, :c])[:8].tolist())
        assert np.array_equal(fc.bits(trk[f][:, :c]), fc.bits(wt[:, :c])), (what, shape, f, "positions")
