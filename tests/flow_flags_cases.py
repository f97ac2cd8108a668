"""The expected side of the flags tests (include/vo_flow_flags.h; test_flow_flags_emulation.py on the CPU emulator,
test_gpu_flow_flags.py on the MI355X), computed by the checker and shared by both.

USE_INITIAL_FLOW: tests/host_check/lk_flags_ref.c -- oracle/orc_lk.c included as it is plus one driver that makes its level loop
start at a guess -- built into a library of its own with the flags of oracle/Makefile (driver()).  Its pin is the first test of
the emulation file: with guess = prev_pts it gives the bytes of orc.calc_optical_flow_pyr_lk.

GET_MIN_EIGENVALS: positions and status are those of a checker call WITHOUT an err vector (lk_level makes the final in-bounds check
only with one): plain_no_err() / driver(want_err=False).  The values are verified by BRACKETING with the checker's own threshold:
for a point that is admissible with D >= FLT_EPSILON (status 1 from calc_optical_flow_pyr_lk(img, img, [p], win, max_level=0,
min_eig=-1)), a value e is the checker's minEig bit for bit iff the same call gives status 1 at min_eig = e and status 0 at
min_eig = nextafter(e, +inf) in f32 -- the checker casts the threshold to f32 and tests minEig < thr.  eig_sets() holds the four
point sets of the issue's table with the counts asserted from the checker's side; check_min_eigenvals() is the comparison."""
import ctypes as C

import numpy as np

import emu_build
import flow_cases as fc
import flow_win_cases as wc
from conftest import vp

FLAG_GUESS, FLAG_EIG = 4, 8
# CFLAGS of oracle/Makefile
CFLAGS = ["-std=c11", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-Wall", "-Wextra", "-Wno-unused-parameter"]
_CACHE = {}


def ref_lib():
    lib = emu_build.shared("lk_flags_ref", cc="gcc", flags=CFLAGS, libs=["-lm"])
    lib.lkf_initial_flow.restype = C.c_int
    return lib


def driver(prev, nxt, pts, guess, win=21, max_level=3, max_count=30, eps=0.01, min_eig=1e-3, want_err=True):
    """the checker started at `guess`: (next [n, 2], status [n], err [n] or None)"""
    prev, nxt = np.ascontiguousarray(prev, np.uint8), np.ascontiguousarray(nxt, np.uint8)
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    out = np.array(guess, np.float32).reshape(-1, 2).copy()
    n = len(pts)
    assert out.shape == pts.shape
    st, err = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.float32)
    h, w = prev.shape
    rc = ref_lib().lkf_initial_flow(vp(prev), vp(nxt), w, h, vp(pts), n, vp(out), vp(st), vp(err) if want_err else None, win, max_level, max_count,
                                    C.c_double(eps), C.c_double(min_eig), 0, 0)
    assert rc >= 0
    return out, st[:n], (err[:n] if want_err else None)


def plain_no_err(orc, prev, nxt, pts, win=21, max_level=3, max_count=30, eps=0.01, min_eig=1e-3):
    """orc_calc_optical_flow_pyr_lk with err == NULL (oracle.py's wrapper always passes one): (next, status, None)"""
    prev, nxt = np.ascontiguousarray(prev, np.uint8), np.ascontiguousarray(nxt, np.uint8)
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    n = len(pts)
    out, st = np.zeros((max(n, 1), 2), np.float32), np.zeros(max(n, 1), np.uint8)
    h, w = prev.shape
    rc = orc.lib().orc_calc_optical_flow_pyr_lk(vp(prev), vp(nxt), w, h, vp(pts), n, vp(out), vp(st), None, win, max_level, max_count,
                                                C.c_double(eps), C.c_double(min_eig), 0, 0)
    assert rc == 0
    return out[:n], st[:n], None


def guess_case(kind, win, lk_max_level, small_seq, orc):
    """L0 -> L1, 596 points, window win, tracked at lk_max_level from a guess:
         "answer": the flags-0 answer at lk_max_level 3 (E = 2) -- a perfect prediction
         "random": prev + uniform(-6, 6), seed 7
    dict(prev, next, pts, guess, win, lk_max_level, max_level = E, want = driver's (next, status, err), plain = the flags-0 checker
    answer at the same depth, want_no_err = the driver without an err vector)"""
    key = ("guess", kind, win, lk_max_level)
    if key not in _CACHE:
        c3 = wc.case("L0-L1", win, small_seq, orc)   # (any odd window of 5 .. 21)
        prev, nxt, pts = c3["prev"], c3["next"], c3["pts"]
        if kind == "answer":
            guess = np.array(c3["want"][0], np.float32)
        else:
            guess = (pts + np.random.default_rng(7).uniform(-6, 6, pts.shape)).astype(np.float32)
        e = wc.depth(480, 160, lk_max_level)
        _CACHE[key] = dict(prev=prev, next=nxt, pts=pts, guess=guess, win=win, lk_max_level=lk_max_level, max_level=e,
                           want=fc.freeze(driver(prev, nxt, pts, guess, win=win, max_level=e)),
                           want_no_err=fc.freeze(driver(prev, nxt, pts, guess, win=win, max_level=e, want_err=False)),
                           plain=fc.freeze(orc.calc_optical_flow_pyr_lk(prev, nxt, pts, win=win, max_level=e)))
    return _CACHE[key]


def guess_premises(c, kind):
    """what makes an implementation that ignores the guess fail: the driver's positions differ in bits from the flags-0 call's"""
    differ = int((fc.bits(c["want"][0]) != fc.bits(c["plain"][0])).any(1).sum())
    assert len(c["pts"]) == 596 and differ >= 500, differ
    if kind == "random":
        assert (c["want"][1] != c["plain"][1]).sum() >= 1, "a status that depends on the start"
    assert (c["want"][1] == 1).sum() >= 400


ADVERSARIAL = (np.nan, np.inf, -np.inf, 1e12, -1e12, -100.0, 3e9, 1e-40)


def adversarial_case(win, small_seq, orc):
    """crop (96 x 64, E = 1): the checker's answer as the guess, with NaN, +inf, -inf, 1e12, -1e12, -100, 3e9 and 1e-40 in the x
    (even points) or y (odd points) coordinate of the first eight"""
    key = ("adversarial", win)
    if key not in _CACHE:
        c = wc.case("crop", win, small_seq, orc)
        guess = np.array(c["want"][0], np.float32)
        with np.errstate(over="ignore"):
            for i, v in enumerate(ADVERSARIAL):
                guess[i, i & 1] = np.float32(v)
        _CACHE[key] = dict(c, guess=guess, want=fc.freeze(driver(c["prev"], c["next"], c["pts"], guess, win=win, max_level=c["max_level"])),
                           plain=c["want"])
    return _CACHE[key]


def adversarial_premises(c):
    nxt, st, _ = c["want"]
    assert st[:8].tolist() == [0, 0, 0, 0, 0, 0, 0, 1], st[:8]
    for i in range(7):   # the propagated value is the position: the guess itself (x 2^-E, then x 2 per level)
        assert fc.bits(nxt[i])[i & 1] == fc.bits(c["guess"][i])[i & 1], i
    if c["win"] == 21:
        assert (st[8:] == 1).sum() == 50 and len(st) == 60


# ---- GET_MIN_EIGENVALS ------------------------------------------------------------------------------------------------------
def admissible(img, pts, win):
    """the level-0 template window of a point is admissible (lk_level: the corner in [-win, w) x [-win, h))"""
    h, w = img.shape
    ip = np.floor(pts - np.float32((win - 1) * 0.5)).astype(np.int64)
    return (ip[:, 0] >= -win) & (ip[:, 0] < w) & (ip[:, 1] >= -win) & (ip[:, 1] < h)


# (set, window) -> points the bracketing can verify; "lattice": of (234, 192) admissible ones
EIG_VERIFIABLE = {("crop60", 21): 60, ("crop60", 9): 60, ("pts596", 21): 596, ("pts596", 9): 596, ("lattice", 21): 204, ("lattice", 9): 150,
                  ("flat", 21): 0, ("flat", 9): 0}
EIG_ADMISSIBLE = {("lattice", 21): 234, ("lattice", 9): 192}
EIG_BELOW_THRESHOLD = {("pts596", 21): 24, ("pts596", 9): 28}


def eig_set(name, win, small_seq, orc):
    """dict(img, pts, win, adm [n] bool, verifiable [n] bool, below [n] bool: verifiable but under the 1e-3 threshold, want_no_err:
    the checker on (img, img) at max_level 0 without an err vector) -- with the table's counts asserted from the checker"""
    key = ("eig", name, win)
    if key not in _CACHE:
        im, ps = fc.images(small_seq), fc.point_sets(small_seq)
        img, pts = {"crop60": (im["cL0"], ps["crop60"]), "pts596": (im["L0"], ps["pts596"]), "lattice": (im["cL0"], ps["lattice"]),
                    "flat": (im["flat"], ps["flat50"])}[name]
        adm = admissible(img, pts, win)
        ver = orc.calc_optical_flow_pyr_lk(img, img, pts, win=win, max_level=0, min_eig=-1.0)[1] == 1
        st3 = orc.calc_optical_flow_pyr_lk(img, img, pts, win=win, max_level=0, min_eig=1e-3)[1] == 1
        assert not (ver & ~adm).any()
        assert int(ver.sum()) == EIG_VERIFIABLE[(name, win)], (name, win, int(ver.sum()))
        if (name, win) in EIG_ADMISSIBLE:
            assert int(adm.sum()) == EIG_ADMISSIBLE[(name, win)]
        elif name != "flat":
            assert adm.all()
        below = ver & ~st3
        if (name, win) in EIG_BELOW_THRESHOLD:
            assert int(below.sum()) == EIG_BELOW_THRESHOLD[(name, win)]
        _CACHE[key] = dict(img=img, pts=pts, win=win, adm=adm, verifiable=ver, below=below,
                           want_no_err=fc.freeze(plain_no_err(orc, img, img, pts, win=win, max_level=0)))
    return _CACHE[key]


def _bracket(orc, img, p, win, e):
    """is the f32 e the checker's minEig of point p, bit for bit (results are remembered: both test files ask the same questions)"""
    key = ("bracket", id(img), win, p.tobytes(), np.float32(e).tobytes())
    if key not in _CACHE:
        up = np.nextafter(np.float32(e), np.float32(np.inf))
        one = p.reshape(1, 2)
        at = orc.calc_optical_flow_pyr_lk(img, img, one, win=win, max_level=0, min_eig=float(np.float32(e)))[1][0]
        above = orc.calc_optical_flow_pyr_lk(img, img, one, win=win, max_level=0, min_eig=float(up))[1][0]
        _CACHE[key] = bool(np.isfinite(e)) and at == 1 and above == 0
    return _CACHE[key]


def check_min_eigenvals(orc, s, got, what=""):
    """got = (next, status, err) of the product on (img, img) at lk_max_level 0 with GET_MIN_EIGENVALS: positions and status are the
    checker's without an err vector, every verifiable value is the checker's by bracketing, every inadmissible point reports 0, and
    a point under the threshold has status 0 and its value"""
    nxt, st, err = got
    fc.assert_same((nxt, st, None), s["want_no_err"], what)
    assert np.all(fc.bits(err[~s["adm"]]) == 0), (what, "an inadmissible level-0 template reports 0")
    bad = [i for i in np.flatnonzero(s["verifiable"]) if not _bracket(orc, s["img"], s["pts"][i], s["win"], err[i])]
    assert not bad, (what, "min eigenvalue differs from the checker's", bad[:8], err[bad[:8]])
    if s["below"].any():
        assert np.all(st[s["below"]] == 0) and np.all(err[s["below"]] != 0) and np.all(err[s["below"]] < np.float32(1e-3)), what
    if not s["verifiable"].any():   # flat
        assert np.all(st == 0) and np.all(fc.bits(err) == 0), what


def final_check_case(small_seq, orc):
    """cL0 -> cL1, flow_cases.lattice(96, 64, step=2.5) (3 618 points), lk_max_count 2, lk_max_level 3 (E = 1), 21 x 21: points whose
    second step leaves the image -- status 1 without an err vector, 0 with one, at identical positions"""
    key = "final-check"
    if key not in _CACHE:
        im = fc.images(small_seq)
        pts = fc.lattice(96, 64, step=2.5)
        with_err = orc.calc_optical_flow_pyr_lk(im["cL0"], im["cL1"], pts, win=21, max_level=1, max_count=2)
        no_err = plain_no_err(orc, im["cL0"], im["cL1"], pts, win=21, max_level=1, max_count=2)
        flips = (no_err[1] == 1) & (with_err[1] == 0)
        assert len(pts) == 3618 and flips.sum() >= 10 and np.array_equal(fc.bits(no_err[0]), fc.bits(with_err[0]))
        assert not ((no_err[1] == 0) & (with_err[1] == 1)).any()
        _CACHE[key] = dict(prev=im["cL0"], next=im["cL1"], pts=pts, win=21, lk_max_level=3, max_level=1, max_count=2, want_no_err=fc.freeze(no_err),
                           with_err=fc.freeze(with_err), flips=flips)
    return _CACHE[key]
