"""Inputs and the checker's answers for the tests of the LK level entry, level set-up and cell test (test_lk_level_setup.py on the
CPU emulator, test_gpu_lk_level_setup.py on the MI355X): 96 x 64 images (one case 96 x 88), about 30 to 50 points per case, every
case crossed with the parameter sets of PARAMS (lk_max_level, lk_max_count, lk_min_eig_threshold; params_of), full chain.

What the set-up of a level decides, and the case that puts solves on each side of it:
  * the template's window test, per level        "outside": x or y in {-100, -60, -25, -20, -15, n + 14, n + 50, n + 170} -- refused at
                                                 level 0 and admitted one level up (-20, -15, n + 14), refused everywhere (the rest)
  * NaN / +-inf coordinates                      "nonfinite"
  * the min-eigenvalue test, shortcut and exact  "flat" (exact test rejects), "faint" (steps of one grey level; the sweep of
                                                 lk_min_eig_threshold puts solves on both sides of the shortcut and of the exact test)
  * D < FLT_EPSILON behind an admitted tensor    "one-way" (a gradient in x only) at threshold 0
  * the largest A's and D                        "checker" (0 / 255 squares)
  * the start of a level: 2^-level * point at the deepest, 2 * out at every other; lk_max_level 0, 2, 3, 4 (at 96 x 64 the plan
    stops at level 1 whatever is asked beyond it -- the next level would not be larger than the window, as in the reference; "deep",
    96 x 88, reaches level 2: a level that is neither the first nor the last)
  * the first cell of a finer level not admitted "jump": the second image at half the contrast, so that the coarse level's first
                                                 step is tens of pixels long
  * lk_max_count 0 (no iteration: out stays the level's start value), 1, 30
  * the template's iw11 = -1                     "iw11": fractional positions found by search through the weights' formula

premises() checks from the checker's logs and a numpy restatement of the reference's level set-up -- never from the library under
test -- that the cases take these paths."""
import ctypes as C

import numpy as np

from conftest import vp
from test_oracle_images import smooth_image

W, H = 96, 64
H_DEEP = 88
WIN = 21
F32 = np.float32
FLT_EPSILON = F32(1.1920929e-07)
# (lk_max_level, lk_max_count, lk_min_eig_threshold).  The thresholds beside 1e-3 sweep the min eigenvalues of "faint", 1.4e-6 ..
# 3.2e-5 by the restatement below: three of them ARE the min eigenvalue (an f32, written out) of one of its templates -- two of
# level 0, one of level 1 --, which the exact test admits ("not below") and the shortcut, with its margin of 1e-3, cannot.
PARAMS = ((0, 30, 1e-3), (2, 30, 1e-3), (3, 30, 1e-3), (4, 30, 1e-3), (2, 0, 1e-3), (2, 1, 1e-3),
          (2, 30, 0.0), (2, 30, 1.1379658644727897e-05), (2, 30, 1.775963573891204e-05), (2, 30, 2.1806947188451886e-05), (2, 30, 1e-4))
CASES = ("outside", "nonfinite", "flat", "faint", "one-way", "checker", "jump", "iw11", "deep")
SWEEP_CASES = ("flat", "faint", "one-way", "checker")     # the cases whose tensors the threshold sweep is about


def params_of(name):
    """the parameter sets the CPU emulator runs a case with (seconds per set there): levels and counts for every case, the
    threshold sweep where the tensor is near a threshold or degenerate.  The GPU test crosses every case with every set."""
    return PARAMS if name in SWEEP_CASES else PARAMS[:6]
LOG_LEVELS = 8
_CACHE = {}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def _shifted(s, h=H, seed=5):
    return [smooth_image(W, h, dx, dy, seed=seed) for dx, dy in ((0.0, 0.0), (s, 0.5 * s), (0.3 * s, -0.4 * s), (0.8 * s, 0.2 * s))]


def _central(h=H):
    xs, ys = np.arange(14.25, 84, 9.9), np.arange(13.6, h - 12, 9.3)
    return np.stack(np.meshgrid(xs, ys), -1).reshape(-1, 2).astype(np.float32)


def weights(a, b):
    """the reference's 14-bit weights of the fractions (a, b), f32 arithmetic: iw00, iw01, iw10, iw11"""
    a, b = F32(a), F32(b)
    s = F32(1 << 14)
    iw00 = int(np.rint(F32(F32(F32(1) - a) * F32(F32(1) - b)) * s))
    iw01 = int(np.rint(F32(a * F32(F32(1) - b)) * s))
    iw10 = int(np.rint(F32(F32(F32(1) - a) * b) * s))
    return iw00, iw01, iw10, (1 << 14) - iw00 - iw01 - iw10


def _iw11_points():
    """points whose level-0 template corner has fractions with iw11 = -1: x = 30 + 2 i + a with a a multiple of 2^-16 (exact in
    f32 below 128, and x - 10 keeps the fraction).  The three rounded weights then sum to 2^14 + 1: a * b * 2^14 below 1/2 and
    every rounding upwards."""
    found = []
    for k in range(3, 2000, 84):
        for l in range(3 + k % 50, 2000):
            if weights(k / 65536.0, l / 65536.0)[3] < 0:
                found.append((k / 65536.0, l / 65536.0) if len(found) % 2 else (l / 65536.0, k / 65536.0))
                break
    assert len(found) >= 16, "the search found too few fraction pairs with iw11 < 0"
    return np.array([(30.0 + 2.0 * (i % 8) + a, 24.0 + 2.0 * (i // 8) + b) for i, (a, b) in enumerate(found) if weights(a, b)[3] < 0], np.float32)


def case(name):
    """dict(imgs = [L0, R0, L1, R1], pts [n, 2], w, h)"""
    if name in _CACHE:
        return _CACHE[name]
    h = H
    if name == "outside":
        imgs = _shifted(1.7)
        off = lambda n: [-100.0, -60.0, -25.0, -20.0, -15.0, n + 14.0, n + 50.0, n + 170.0]
        pts = np.vstack([[(x, y) for x in off(W) for y in (20.6, 41.1)], [(x, y) for y in off(H) for x in (30.3, 61.7)],
                         [(-15.0, -15.0), (W + 14.0, H + 14.0), (-20.0, H + 14.0)], _central()[::3]]).astype(np.float32)
    elif name == "nonfinite":
        imgs = _shifted(1.7)
        odd = [(np.nan, 20.0), (20.0, np.nan), (np.nan, np.nan), (np.inf, 20.0), (20.0, np.inf), (-np.inf, 20.0), (20.0, -np.inf),
               (np.inf, -np.inf), (3e38, 20.0), (20.0, -3e38), (np.nan, np.inf)]
        pts = np.vstack([odd, _central()[:36]]).astype(np.float32)
    elif name == "flat":
        imgs = _shifted(1.7, seed=6)
        for im in imgs:
            im[8:58, 22:76] = 97
        pts = np.vstack([np.stack(np.meshgrid(np.arange(40.3, 60, 6.1), np.arange(26.4, 40, 4.2)), -1).reshape(-1, 2), _central()[::2]]).astype(np.float32)
    elif name == "faint":
        # steps of one grey level every 24 columns and every 16 rows, and a second, sparser set the other way: every window sees
        # one or two steps in each direction, min eigenvalues around 1e-4 (premises)
        ys, xs = np.mgrid[0:H, 0:W]
        im = (100 + xs // 24 + ys // 16 + ((xs + 2 * ys) // 37) % 2).astype(np.uint8)
        imgs, pts = [im, im.copy(), im.copy(), im.copy()], _central()
    elif name == "one-way":
        ys, xs = np.mgrid[0:H, 0:W]
        im = (40 + 2 * xs).astype(np.uint8)       # Iy = 0 everywhere: A12 = A22 = 0, D = 0, min eigenvalue 0
        imgs, pts = [im, im.copy(), im.copy(), im.copy()], _central()
    elif name == "checker":
        ys, xs = np.mgrid[0:H, 0:W]
        im = (255 * (((xs // 3) + (ys // 3)) % 2)).astype(np.uint8)
        imgs, pts = [im, im.copy(), im.copy(), im.copy()], _central()
    elif name == "jump":
        # R0 is L0 at half the contrast plus an offset: the first Gauss-Newton step of the coarse level is tens of pixels long, the
        # level ends outside, and twice that is no corner level 0 admits -- its first cell is refused before any iteration
        im = smooth_image(W, H, seed=9)
        dim = (im // 2 + 40).astype(np.uint8)
        imgs = [im, dim, dim.copy(), im.copy()]
        pts = np.stack(np.meshgrid(np.arange(3.3, 96, 7.7), np.arange(2.6, 64, 6.9)), -1).reshape(-1, 2)[::4].astype(np.float32)
    elif name == "iw11":
        imgs, pts = _shifted(0.3), np.vstack([_iw11_points(), _central()[::2]]).astype(np.float32)
    elif name == "deep":
        h = H_DEEP
        imgs, pts = _shifted(2.9, h=h, seed=12), np.vstack([_central(h)[::2], [(-15.0, 30.0), (W + 14.0, 40.0), (50.0, -30.0)]]).astype(np.float32)
    else:
        raise KeyError(name)
    _CACHE[name] = dict(imgs=[_frozen(im) for im in imgs], pts=_frozen(pts), w=W, h=h)
    return _CACHE[name]


def oracle(orc, name, prm):
    """the checker's four hops with its iteration log: dict(trk [4, n, 2], status [4, n], iters [4, LOG_LEVELS, n] (-1: the solve
    was not reached))"""
    key = ("oracle", name, prm)
    if key not in _CACHE:
        c = case(name)
        l0, r0, l1, r1 = c["imgs"]
        p, n = c["pts"], len(c["pts"])
        max_level, max_count, min_eig = prm
        lib = orc.lib()
        trk, st, its = [], [], []
        try:
            for a, b in ((l0, r0), (r0, r1), (r1, l1), (l1, l0)):
                it = np.full((LOG_LEVELS, n), -1, np.int32)
                lib.orc_lk_set_iteration_log(vp(it), C.c_int(n))
                p, s, _ = orc.calc_optical_flow_pyr_lk(a, b, p, max_level=max_level, max_count=max_count, min_eig=min_eig)
                trk.append(p)
                st.append(s)
                its.append(it)
        finally:
            lib.orc_lk_set_iteration_log(None, C.c_int(0))
        _CACHE[key] = dict(trk=_frozen(np.stack(trk)), status=_frozen(np.stack(st)), iters=_frozen(np.stack(its)))
    return _CACHE[key]


def oracle_flow(orc, name, prm, win, pair=(0, 1)):
    """the checker's one hop between two images of the case, with err: (next, status, err)"""
    key = ("flow", name, prm, win, pair)
    if key not in _CACHE:
        c = case(name)
        max_level, max_count, min_eig = prm
        _CACHE[key] = tuple(_frozen(x) for x in orc.calc_optical_flow_pyr_lk(c["imgs"][pair[0]], c["imgs"][pair[1]], c["pts"], win=win,
                                                                               max_level=max_level, max_count=max_count, min_eig=min_eig))
    return _CACHE[key]


def assert_chain(got_trk, got_st, want, what):
    """status on every hop; positions as raw bits on every hop the checker reports alive"""
    assert np.array_equal(got_st, want["status"]), (what, "status", np.argwhere(got_st != want["status"])[:8].tolist())
    alive = want["status"] == 1
    same = (bits(got_trk) == bits(want["trk"])).all(-1)
    assert same[alive].all(), (what, "positions", np.argwhere(alive & ~same)[:8].tolist())


# ---- the reference's level set-up, restated in numpy (lkpyramid.cpp, LKTrackerInvoker: the template of one point at one level) ----
def depth(h, max_level, w=W):
    """the deepest level: the pyramid stops where the next level would not be larger than the window"""
    l = 0
    while l < max_level and (w + 1) // 2 > WIN and (h + 1) // 2 > WIN:
        w, h, l = (w + 1) // 2, (h + 1) // 2, l + 1
    return l


def _level(orc, name, level):
    key = ("level", name, level)
    if key not in _CACHE:
        im = orc.build_pyramid(case(name)["imgs"][0], level)[level]
        d = orc.scharr(im).astype(np.int64)
        pad = WIN + 2
        _CACHE[key] = (im.shape, np.pad(im.astype(np.int64), pad, mode="reflect"), np.pad(d, ((pad, pad), (pad, pad), (0, 0))), pad)
    return _CACHE[key]


def setup(orc, name, level, pt, min_eig):
    """what the reference's set-up of `level` does with hop 0's point `pt`: dict(window (the template's window is admitted), iw11,
    A11, A12, A22, D, min_eig, shortcut (the kernel's sufficient test admits without the square root), admitted (the exact
    min-eigenvalue test), solve (admitted and D >= FLT_EPSILON))"""
    (h, w), _, d, pad = _level(orc, name, level)
    half = F32((WIN - 1) * 0.5)
    px, py = (F32(F32(v) * F32(1.0 / (1 << level))) - half for v in pt)
    out = dict(window=False, solve=False)
    if not (np.isfinite(px) and np.isfinite(py)):
        return out
    ipx, ipy = int(np.floor(px)), int(np.floor(py))
    if ipx < -WIN or ipx >= w or ipy < -WIN or ipy >= h:
        return out
    iw = weights(px - F32(ipx), py - F32(ipy))
    y0, x0 = ipy + pad, ipx + pad
    win = lambda dy, dx: d[y0 + dy:y0 + dy + WIN, x0 + dx:x0 + dx + WIN]
    v = (win(0, 0) * iw[0] + win(0, 1) * iw[1] + win(1, 0) * iw[2] + win(1, 1) * iw[3] + (1 << 13)) >> 14
    scale = F32(1.0 / (1 << 20))
    A11, A12, A22 = (F32(F32(int(s)) * scale) for s in ((v[..., 0] ** 2).sum(), (v[..., 0] * v[..., 1]).sum(), (v[..., 1] ** 2).sum()))
    D = F32(F32(A11 * A22) - F32(A12 * A12))
    t = F32(A22 + A11)
    s2 = F32(F32(F32(A11 - A22) * F32(A11 - A22)) + F32(F32(F32(4) * A12) * A12))
    me = F32(F32(t - np.sqrt(s2)) / F32(2 * WIN * WIN))
    thr = F32(min_eig)
    u = F32(t - F32(F32(thr * F32(F32(1.001) * F32(2 * WIN * WIN))) + F32(t * F32(3.814697265625e-6))))
    shortcut = bool(u > 0 and s2 < F32(F32(u * u) * F32(0.9999)))
    admitted = not (me < thr)
    assert admitted or not shortcut, "the shortcut admits what the exact test rejects"
    out.update(window=True, iw11=iw[3], A11=A11, A12=A12, A22=A22, D=D, min_eig=me, shortcut=shortcut, admitted=admitted,
               solve=bool(admitted and not (D < FLT_EPSILON)))
    return out


def premises(orc):
    """the cases take the paths they are there for; returns the counts"""
    seen = dict(refused_then_admitted=0, refused_everywhere=0, nonfinite=0, shortcut=0, exact_admits=0, exact_rejects=0, small_D=0,
                largest_A=0.0, first_cell_refused=0, no_iteration=0, one_iteration=0, iw11=0, middle_level=0)
    for name in CASES:
        c = case(name)
        for prm in PARAMS:
            max_level, max_count, min_eig = prm
            top = depth(c["h"], max_level)
            o = oracle(orc, name, prm)
            for i, pt in enumerate(c["pts"]):
                s = [setup(orc, name, l, pt, min_eig) for l in range(top + 1)]
                # the restatement and the checker agree on which solves were reached (hop 0)
                for l in range(top + 1):
                    assert (o["iters"][0, l, i] >= 0) == s[l]["solve"], (name, prm, i, l, s[l], o["iters"][0, :, i])
                if not np.isfinite(pt).all():
                    seen["nonfinite"] += 1
                    assert o["status"][0, i] == 0
                    continue
                if top >= 1 and not s[0]["window"]:
                    seen["refused_then_admitted" if any(x["window"] for x in s[1:]) else "refused_everywhere"] += 1
                    assert o["status"][0, i] == 0
                for l, x in enumerate(s):
                    if not x["window"]:
                        continue
                    seen["shortcut"] += x["shortcut"]
                    seen["exact_admits"] += (not x["shortcut"]) and x["admitted"]
                    seen["exact_rejects"] += not x["admitted"]
                    seen["small_D"] += x["admitted"] and not x["solve"]
                    seen["largest_A"] = max(seen["largest_A"], float(x["A11"]), float(x["A22"]))
                    seen["iw11"] += x["iw11"] < 0
                    seen["middle_level"] += x["solve"] and 0 < l < top
                it0 = o["iters"][0, 0, i]
                if max_count == 30 and top >= 1 and it0 == 0:
                    seen["first_cell_refused"] += 1          # the solve was reached, the first corner was outside: status 0
                    assert o["status"][0, i] == 0
                if max_count == 0 and it0 == 0 and o["status"][0, i] == 1:
                    seen["no_iteration"] += 1
                if max_count == 1 and it0 == 1:
                    seen["one_iteration"] += 1
    assert all(v > 0 for v in seen.values()), seen
    assert seen["largest_A"] > 2048, seen       # the checkerboard: A's within a factor of 8 of the wave sums' 2^14
    # lk_max_count = 0: no iteration at any level, so hop 0 of a live point ends where it started, bit for bit
    for name in ("checker", "deep"):
        o, p = oracle(orc, name, (2, 0, 1e-3)), case(name)["pts"]
        live = o["status"][0] == 1
        assert live.any() and (bits(o["trk"][0])[live] == bits(p)[live]).all()
    return seen
