"""Inputs and expected results of the windowed two-image tracker (include/vo_flow_win.h): tests/flow_cases.py's images and point
sets with a window W, a start-point lattice that scales with it, and the checker's answer
    orc.calc_optical_flow_pyr_lk(prev, next, pts, win=W, max_level=E)                       (accum_mode 0)
for each, computed once per session and never modified.  E is the depth contract of vo_flow_win.h: the deepest level the library
plans for the image size under its lk_max_level -- levels stay larger than 21 pixels whatever the window -- restated here
(depth) and compared with vowin_max_level on the device.  premises() is what every comparison asserts first, on the checker's
side alone: the floors were taken from the checker for every odd W of 5 .. 19 before any kernel existed."""
import numpy as np

import flow_cases as fc

WINDOWS = (5, 7, 9, 11, 13, 15, 17, 19)
_CACHE = {}


def depth(w, h, lk_max_level, max_levels=5):
    """E: the deepest pyramid level index for a w x h image (capi.hip: plan_levels -- stop when the next level would not be larger
    than 21 x 21, at lk_max_level, or at the library's five levels)"""
    lvl = 0
    while lvl < lk_max_level and lvl + 1 < max_levels and (w + 1) // 2 > 21 and (h + 1) // 2 > 21:
        w, h, lvl = (w + 1) // 2, (h + 1) // 2, lvl + 1
    return lvl


def lattice(w, h, win, step=6.5):
    """start points from -(W + 9) to w + W + 19 and -(W + 9) to h + W + 19: both sides of the +-W admissibility window and of the
    final bounds check, for every window"""
    xs = np.arange(-(win + 9.0), w + win + 19.0 + 1e-3, step, dtype=np.float32)
    ys = np.arange(-(win + 9.0), h + win + 19.0 + 1e-3, step, dtype=np.float32)
    return np.stack(np.meshgrid(xs, ys), -1).reshape(-1, 2).astype(np.float32)


# name -> (prev image, next image, point set, lk_max_level of the context)
CASES = {
    "L0-L1": ("L0", "L1", "pts596", 3),
    "L0-R0": ("L0", "R0", "pts596", 3),
    "L0-L1-level0": ("L0", "L1", "pts596", 0),
    "crop": ("cL0", "cL1", "crop60", 3),
    "lattice": ("cL0", "cL1", "lattice", 3),
    "flat": ("flat", "flat", "flat50", 3),
}


def case(name, win, small_seq, orc):
    """dict(prev, next, pts, win, lk_max_level, max_level = E, want = (next, status, err))"""
    key = (name, win)
    if key not in _CACHE:
        a, b, p, ml = CASES[name]
        im = fc.images(small_seq)
        pts = lattice(96, 64, win) if p == "lattice" else fc.point_sets(small_seq)[p]
        h, w = im[a].shape
        e = depth(w, h, ml)
        want = fc.freeze(orc.calc_optical_flow_pyr_lk(im[a], im[b], pts, win=win, max_level=e))
        _CACHE[key] = dict(prev=im[a], next=im[b], pts=pts, win=win, lk_max_level=ml, max_level=e, want=want)
    return _CACHE[key]


def premises(name, c):
    """the checker's side of a comparison (the issue's table of floors)"""
    nxt, st, err = c["want"]
    n1, n0 = int((st == 1).sum()), int((st == 0).sum())
    assert np.all(err[st == 0] == 0), "err of a status-0 point is exactly 0"
    if name != "flat":
        assert np.all(err[st == 1] > 0), "a moving pair: non-zero err on every tracked point"
    if name in ("L0-L1", "L0-R0"):
        assert len(st) == 596 and c["max_level"] == 2 and n1 >= 500 and n0 >= 30, (name, c["win"], n1, n0)
        if name == "L0-R0":
            assert ((st == 1) & ((nxt < 0).any(1))).sum() >= 1, "a tracked point that left the image"
    elif name == "L0-L1-level0":
        assert len(st) == 596 and c["max_level"] == 0 and n1 >= 500 and n0 >= 20, (name, c["win"], n1, n0)
    elif name == "crop":
        assert len(st) == 60 and c["max_level"] == 1 and n1 >= 40 and n0 >= 1, (name, c["win"], n1, n0)
    elif name == "lattice":
        assert c["max_level"] == 1 and n1 >= 60 and n0 >= 200, (name, c["win"], n1, n0)
    elif name == "flat":
        assert n1 == 0 and n0 == len(st) > 0


def depth_premise(win, small_seq, orc):
    """number of points of L0-L1 whose bits differ between the checker at max_level 3 (what OpenCV would build for a window below
    21 on 480 x 160) and at E = 2 (what the library tracks on): a test that passes the wrong depth fails"""
    key = ("depth", win)
    if key not in _CACHE:
        c = case("L0-L1", win, small_seq, orc) if win != 21 else None
        im, pts = fc.images(small_seq), fc.point_sets(small_seq)["pts596"]
        at2 = c["want"] if c else orc.calc_optical_flow_pyr_lk(im["L0"], im["L1"], pts, win=win, max_level=2)
        at3 = orc.calc_optical_flow_pyr_lk(im["L0"], im["L1"], pts, win=win, max_level=3)
        _CACHE[key] = int((fc.bits(at2[0]) != fc.bits(at3[0])).any(1).sum())
    return _CACHE[key]


def window_premise(win, small_seq, orc):
    """number of points of L0-L1 whose expected position differs from the 21 x 21 one at the same depth: a window that is silently
    ignored fails"""
    key = ("window", win)
    if key not in _CACHE:
        c = case("L0-L1", win, small_seq, orc)
        w21 = orc.calc_optical_flow_pyr_lk(c["prev"], c["next"], c["pts"], win=21, max_level=c["max_level"])
        _CACHE[key] = int((fc.bits(c["want"][0]) != fc.bits(w21[0])).any(1).sum())
    return _CACHE[key]


N_RANDOM = 16


def random_case(seed, small_seq, orc):
    """flow_cases.random_case -- crops of 64 .. 200 x 48 .. 160 of L0 -> L1, n of 0 .. 128 points uniform in [-25, w + 25] x
    [-25, h + 25], lk_max_level of 0 .. 4 -- with a random odd window: the 16 seeds walk a shuffled list that holds each window
    twice, so every window is drawn"""
    key = ("random", seed)
    if key not in _CACHE:
        order = np.random.default_rng(77).permutation(np.repeat(WINDOWS, 2))
        assert 0 <= seed < N_RANDOM == len(order)
        win = int(order[seed])
        prev, nxt, pts, ml = fc.random_draw(np.random.default_rng(2000 + seed), seed, small_seq)
        e = depth(prev.shape[1], prev.shape[0], ml)
        want = orc.calc_optical_flow_pyr_lk(prev, nxt, pts, win=win, max_level=e) if len(pts) else fc.no_points()
        _CACHE[key] = dict(prev=prev, next=nxt, pts=pts, win=win, lk_max_level=ml, max_level=e, want=fc.freeze(want))
    return _CACHE[key]
