"""Inputs and the checker's answers for the tests of every way out of the LK iteration (test_lk_iteration_paths.py on the CPU
emulator, test_gpu_lk_iteration_paths.py on the MI355X): 96 x 64 images, maxLevel 2, about 40 points per case, every case crossed
with max_count in {1, 2, 30} and epsilon in {1e-30, 0.01, 10}.

epsilon = 10 ends every solve at its first iteration, epsilon = 1e-30 leaves the count and the oscillation test (and a delta of
exactly zero), max_count = 1 ends at the count before any cell test.  The checker's four hops are computed once per session with its
iteration log and cycle log switched on, and never modified: the logs say how each (hop, level, point) solve ended."""
import ctypes as C

import numpy as np

from conftest import vp
from test_oracle_images import smooth_image

W, H = 96, 64
MAX_LEVEL = 2
MAX_COUNTS = (1, 2, 30)
EPSILONS = (1e-30, 0.01, 10.0)
SHIFTS = (0.3, 1.7, 6.2)
CASES = ("identical", "shift-0.3", "shift-1.7", "shift-6.2", "noise", "borders", "flat", "nan-negative")
LOG_LEVELS = 8
_CACHE = {}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def _shifted(s, seed=5):
    """L0, R0, L1, R1: hops of (s, s / 2), (-0.2 s, -0.3 s), (-0.5 s, -0.6 s), (-0.3 s, 0.4 s)"""
    return [smooth_image(W, H, dx, dy, seed=seed) for dx, dy in ((0.0, 0.0), (s, 0.5 * s), (0.3 * s, -0.4 * s), (0.8 * s, 0.2 * s))]


def _central():
    xs, ys = np.arange(14.25, 84, 9.9), np.arange(13.6, 52, 9.3)
    return np.stack(np.meshgrid(xs, ys), -1).reshape(-1, 2).astype(np.float32)


def _border_points():
    """within 12 pixels of every border, the corners included"""
    near = lambda n: [0.0, 0.5, 3.3, 7.9, 11.5, n - 12.5, n - 8.2, n - 3.7, n - 1.5, n - 1.0]
    along = lambda n: list(np.arange(6.4, n - 4, 17.3))
    top = [(x, y) for x in along(W) for y in (0.5, 7.9, H - 8.2, H - 1.0)]
    side = [(x, y) for x in near(W) for y in (20.6, 41.1)]
    return np.array(top + side, np.float32)


def case(name):
    """dict(imgs = [L0, R0, L1, R1], pts [n, 2])"""
    if name in _CACHE:
        return _CACHE[name]
    if name == "identical":
        im = smooth_image(W, H, seed=5)
        imgs, pts = [im, im, im, im], _central()
    elif name.startswith("shift-"):
        imgs, pts = _shifted(float(name[6:])), _central()
    elif name == "noise":
        rng = np.random.default_rng(20)
        imgs, pts = [rng.integers(0, 256, (H, W), dtype=np.uint8) for _ in range(4)], _central()
    elif name == "borders":
        imgs, pts = _shifted(6.2, seed=8), _border_points()
    elif name == "flat":
        imgs = _shifted(1.7, seed=6)
        for im in imgs:
            im[8:58, 22:76] = 97          # a patch that holds whole windows: no gradient, the min-eigenvalue test rejects
        pts = np.vstack([np.stack(np.meshgrid(np.arange(40.3, 60, 6.1), np.arange(26.4, 40, 4.2)), -1).reshape(-1, 2), _central()[::2]]).astype(np.float32)
    elif name == "nan-negative":
        imgs = _shifted(1.7)
        pts = np.vstack([_central()[:38], [[np.nan, 20.0]], [[-3.0, 20.5]]]).astype(np.float32)
    else:
        raise KeyError(name)
    _CACHE[name] = dict(imgs=[_frozen(im) for im in imgs], pts=_frozen(pts))
    return _CACHE[name]


def oracle(orc, name, max_count, eps):
    """the checker's four hops with its logs: dict(trk [4, n, 2], status [4, n], iters [4, LOG_LEVELS, n] (-1: the solve was not
    reached), cycle [4, LOG_LEVELS, n, 2])"""
    key = ("oracle", name, max_count, eps)
    if key not in _CACHE:
        c = case(name)
        l0, r0, l1, r1 = c["imgs"]
        p, n = c["pts"], len(c["pts"])
        lib = orc.lib()
        trk, st, its, cyc = [], [], [], []
        try:
            for a, b in ((l0, r0), (r0, r1), (r1, l1), (l1, l0)):
                it = np.full((LOG_LEVELS, n), -1, np.int32)
                cy = np.zeros((LOG_LEVELS, n, 2), np.int32)
                lib.orc_lk_set_iteration_log(vp(it), C.c_int(n))
                lib.orc_lk_set_cycle_log(vp(cy))
                p, s, _ = orc.calc_optical_flow_pyr_lk(a, b, p, max_level=MAX_LEVEL, max_count=max_count, eps=eps)
                trk.append(p)
                st.append(s)
                its.append(it)
                cyc.append(cy)
        finally:
            lib.orc_lk_set_cycle_log(None)
            lib.orc_lk_set_iteration_log(None, C.c_int(0))
        _CACHE[key] = dict(trk=_frozen(np.stack(trk)), status=_frozen(np.stack(st)), iters=_frozen(np.stack(its)), cycle=_frozen(np.stack(cyc)))
    return _CACHE[key]


FLOW_PAIR = (1, 2)  # the two-image call's images of a case: R0 -> L1, the pair of the border case that pushes windows out of the image


def oracle_flow(orc, name, max_count, eps):
    """the checker's one hop between the images FLOW_PAIR of the case, with err: (next, status, err)"""
    key = ("flow", name, max_count, eps)
    if key not in _CACHE:
        c = case(name)
        a, b = (c["imgs"][i] for i in FLOW_PAIR)
        _CACHE[key] = tuple(_frozen(x) for x in orc.calc_optical_flow_pyr_lk(a, b, c["pts"], max_level=MAX_LEVEL, max_count=max_count, eps=eps))
    return _CACHE[key]


def assert_chain(got_trk, got_st, want, what):
    """status on every hop; positions as raw bits on every hop the checker reports alive"""
    assert np.array_equal(got_st, want["status"]), (what, "status", np.argwhere(got_st != want["status"])[:8].tolist())
    alive = want["status"] == 1
    same = (bits(got_trk) == bits(want["trk"])).all(-1)
    assert same[alive].all(), (what, "positions", np.argwhere(alive & ~same)[:8].tolist())


def premises(orc):
    """what the sweep must hold for the comparisons to mean something, from the checker alone"""
    # a comparison must not pass by being empty: on each shifted pair with the default parameters at least half the points
    # are alive through hop 3
    for s in SHIFTS:
        st = oracle(orc, "shift-%s" % s, 30, 0.01)["status"]
        assert (st == 1).all(0).sum() * 2 >= st.shape[1], (s, (st == 1).all(0).sum())
    # the flat patch is rejected by the min-eigenvalue test (no iteration at level 0), the NaN and the negative point fail hop 0
    flat = oracle(orc, "flat", 30, 0.01)
    assert ((flat["status"][0, :12] == 0) & (flat["iters"][0, 0, :12] == -1)).all() and (flat["status"][0, 12:] == 1).any()
    odd = oracle(orc, "nan-negative", 30, 0.01)
    assert odd["status"][0, -2] == 0 and (odd["status"][0, :38] == 1).sum() >= 19
    # every way out of the loop, at least once over the sweep
    seen = dict(epsilon=0, oscillation=0, count=0, left=0)
    for name in CASES:
        for mc in MAX_COUNTS:
            for eps in EPSILONS:
                o = oracle(orc, name, mc, eps)
                it0, alive = o["iters"][:, 0], o["status"] == 1
                # level 0, status 1: the loop was not left through the image test.  One iteration where two were allowed: no
                # oscillation test yet (j = 0), not the count -- epsilon
                if mc >= 2:
                    seen["epsilon"] += int((alive & (it0 == 1)).sum())
                # epsilon out of reach, fewer iterations than allowed, more than one, the corner never repeated (so the last
                # delta was not exactly zero, the one thing epsilon = 1e-30 still catches): the oscillation test
                if eps == 1e-30 and mc == 30:
                    seen["oscillation"] += int((alive & (it0 > 1) & (it0 < mc) & (o["cycle"][:, 0, :, 1] == 0)).sum())
                # status 0 behind at least one iteration of level 0: the window left the image
                seen["left"] += int((~alive & (it0 >= 1)).sum())
    # the count: hop 0 starts from the same points whatever the parameters, and its coarsest level from nothing else -- a solve
    # that runs more than 2 iterations when 30 are allowed and exactly 2 when 2 are was ended by the count
    for name in CASES:
        a, b = oracle(orc, name, 2, 1e-30)["iters"][0], oracle(orc, name, 30, 1e-30)["iters"][0]
        top = max(l for l in range(LOG_LEVELS) if (b[l] >= 0).any())
        assert top >= 1, "one level: maxLevel 2 was meant to give a coarse one"
        seen["count"] += int(((a[top] == 2) & (b[top] > 2)).sum())
    assert all(v > 0 for v in seen.values()), seen
    return seen
