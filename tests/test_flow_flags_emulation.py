"""The two-image tracker's kernels with flags (visual_odom_amd/csrc/lk.hip: lk_flow_flags_kernel<W>, every odd W of 5 .. 21)
executed on the CPU through the coroutine SIMT emulator (tests/host_check/hip_emu.h + flow_emu.cpp, run through
tests/flow_emu.py), from the product source.  The expected side is the checker's (tests/flow_flags_cases.py): for USE_INITIAL_FLOW the
checker's own level loop started at the guess (tests/host_check/lk_flags_ref.c; its pin is the first test here), for
GET_MIN_EIGENVALS the checker without an err vector and its threshold as a bracket around every value.  Positions, status and err
are compared BIT FOR BIT, every point (NaN included), after the premises that make a guess-ignoring or epilogue-keeping kernel fail.

The sanitizer tier is the same harness as a STAND-ALONE program (flow_emu.run_standalone).  Unit test of device code, not a
product path."""
import ctypes as C

import numpy as np
import pytest

import flow_cases as fc
import flow_emu as fe
import flow_flags_cases as gc
import flow_win_cases as wc
from conftest import vp

ALL_WINDOWS = wc.WINDOWS + (21,)
GUESS, EIG = gc.FLAG_GUESS, gc.FLAG_EIG


@pytest.fixture(scope="module")
def femu():
    return fe.load()


def ff_track(lib, c, flags, guess=None, want_err=True, counts=None, max_count=30):
    """the case's pair through the emulated kernel of its window and flags, with the context's lk_max_level; one frame, or
    len(counts) frames of one launch: (next [F, n, 2], status [F, n], err [F, n] or None), F squeezed away for one frame"""
    got, levels = fe.track(lib, c, flags, guess=guess, want_err=want_err, counts=counts, frame=0 if counts is None else None, max_count=max_count)
    assert levels == c["max_level"] + 1, "the harness plans the levels the depth rule says"
    return got


# ---- the expected side's own pin ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(fc.CASES))
def test_driver_with_guess_equal_prev_is_the_checker(orc, small_seq, name):
    """the driver of lk_flags_ref.c started at prev_pts gives the bytes of orc.calc_optical_flow_pyr_lk: every window, every
    flow_cases case, with and without an err vector"""
    a, b, p, ml = fc.CASES[name]
    im, pts = fc.images(small_seq), fc.point_sets(small_seq)[p]
    for win in ALL_WINDOWS:
        want = orc.calc_optical_flow_pyr_lk(im[a], im[b], pts, win=win, max_level=ml)
        fc.assert_same(gc.driver(im[a], im[b], pts, pts, win=win, max_level=ml), want, (name, win))
        fc.assert_same(gc.driver(im[a], im[b], pts, pts, win=win, max_level=ml, want_err=False),
                       gc.plain_no_err(orc, im[a], im[b], pts, win=win, max_level=ml), (name, win, "no err"))


# ---- USE_INITIAL_FLOW ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["crop", "lattice", "L0-L1"])
@pytest.mark.parametrize("win", [5, 9, 15, 21])
def test_guess_equal_prev_gives_the_flags_0_bytes(femu, orc, small_seq, win, name):
    """the flags-0 kernel's bytes are the checker's (test_flow_win_emulation.py, test_flow_emulation.py; run here on crop as well)"""
    c = wc.case(name, win, small_seq, orc)   # (any odd window of 5 .. 21)
    if name == "crop":
        fc.assert_same(ff_track(femu, c, 0), c["want"], (name, win, "flags 0"))
    fc.assert_same(ff_track(femu, c, GUESS, guess=c["pts"]), c["want"], (name, win))


@pytest.mark.parametrize("win,level", [(21, 0), (21, 3), (9, 0)])
def test_guess_is_the_answer(femu, orc, small_seq, win, level):
    """a perfect prediction, tracked on one level and on all: bit for bit the driver; >= 500 of 596 positions differ from flags 0"""
    c = gc.guess_case("answer", win, level, small_seq, orc)
    gc.guess_premises(c, "answer")
    fc.assert_same(ff_track(femu, c, GUESS, guess=c["guess"]), c["want"], ("answer", win, level))


@pytest.mark.parametrize("win", [21, 13])
def test_random_guess(femu, orc, small_seq, win):
    c = gc.guess_case("random", win, 3, small_seq, orc)
    gc.guess_premises(c, "random")
    fc.assert_same(ff_track(femu, c, GUESS, guess=c["guess"]), c["want"], ("random", win))


@pytest.mark.parametrize("win", [21, 7])
def test_adversarial_guesses(femu, orc, small_seq, win):
    """NaN, +-inf, beyond int32, far outside: status 0 and the propagated value as the position, compared by bits"""
    c = gc.adversarial_case(win, small_seq, orc)
    gc.adversarial_premises(c)
    fc.assert_same(ff_track(femu, c, GUESS, guess=c["guess"]), c["want"], ("adversarial", win))


def test_frames_of_one_launch(femu, orc, small_seq):
    """three frames with 60, 0 and 23 points and their own guesses in one launch; rows beyond a frame's count stay untouched"""
    c = gc.adversarial_case(9, small_seq, orc)
    n = len(c["pts"])
    g = np.stack([c["guess"], c["guess"] + 100, c["pts"]])
    nxt, st, err = ff_track(femu, c, GUESS, guess=g, counts=[n, 0, 23])
    fc.assert_same((nxt[0], st[0], err[0]), c["want"], "frame 0")
    assert np.array_equal(fc.bits(nxt[1]), fc.bits(g[1])) and np.all(st[1] == 0xA5) and np.all(err[1] == -1), "frame 1 has no points"
    fc.assert_same((nxt[2, :23], st[2, :23], err[2, :23]), tuple(a[:23] for a in c["plain"]), "frame 2: guess = prev")
    assert np.array_equal(fc.bits(nxt[2, 23:]), fc.bits(g[2, 23:])) and np.all(st[2, 23:] == 0xA5)


# ---- GET_MIN_EIGENVALS --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["crop60", "pts596", "lattice", "flat"])
@pytest.mark.parametrize("win", [21, 9])
def test_min_eigenvalues_by_bracketing(femu, orc, small_seq, win, name):
    s = gc.eig_set(name, win, small_seq, orc)
    c = dict(prev=s["img"], next=s["img"], pts=s["pts"], win=win, lk_max_level=0, max_level=0)
    gc.check_min_eigenvals(orc, s, ff_track(femu, c, EIG), (name, win))


def test_min_eigenvalues_skip_the_final_check(femu, orc, small_seq):
    """>= 10 points of the 2.5-pixel lattice end outside the image: status 1 with the flag (and with err == NULL), 0 without"""
    c = gc.final_check_case(small_seq, orc)
    nxt, st, err = ff_track(femu, c, EIG, max_count=2)
    fc.assert_same((nxt, st, None), c["want_no_err"], "lattice 2.5")
    assert (st[c["flips"]] == 1).all()
    adm = gc.admissible(c["prev"], c["pts"], 21)
    assert np.all(fc.bits(err[~adm]) == 0) and (err[adm] > 0).sum() >= 1000
    k = np.flatnonzero(c["flips"])   # the same points alone: the flag without an err vector, and flags 0
    sub = dict(c, pts=np.ascontiguousarray(c["pts"][k]))
    fc.assert_same(ff_track(femu, sub, EIG, want_err=False, max_count=2), tuple(a[k] for a in c["want_no_err"][:2]) + (None,), "err == NULL")
    fc.assert_same(ff_track(femu, sub, 0, max_count=2), tuple(a[k] for a in c["with_err"]), "flags 0")


def test_both_flags(femu, orc, small_seq):
    """L0 -> L1 from the answer on one level: the driver's positions, the status of a call without an err vector, and the values
    of the min-eigenvalue call on the same template"""
    c = gc.guess_case("answer", 21, 0, small_seq, orc)
    gc.guess_premises(c, "answer")
    nxt, st, err = ff_track(femu, c, GUESS | EIG, guess=c["guess"])
    fc.assert_same((nxt, st, None), c["want_no_err"], "both flags")
    s = gc.eig_set("pts596", 21, small_seq, orc)
    bad = [i for i in range(596) if not gc._bracket(orc, s["img"], s["pts"][i], 21, err[i])]
    assert not bad, bad[:8]


def test_flags_without_a_kernel_are_refused(femu):
    img = np.zeros((64, 96), np.uint8)
    pts = np.zeros((1, 2), np.float32)
    io, st = np.zeros((1, 2), np.float32), np.zeros(1, np.uint8)
    for win, flags in ((21, 1), (21, 2), (21, 16), (21, -1), (20, 4), (23, 8)):
        assert femu.fe_track(vp(img), vp(img), 96, 64, 3, vp(pts), 1, win, flags, 30, C.c_double(0.01), C.c_float(1e-3), vp(io), vp(st), None, 1, None) == -1


@pytest.mark.sanitize
def test_flags_kernels_standalone_under_sanitizers(tmp_path, orc, small_seq):
    """ASan + UBSan over the kernel source in a program of its own: exactly sized pyramid levels, far-off starts, no report, the
    same bits"""
    runs = [(gc.adversarial_case(win, small_seq, orc), GUESS) for win in (21, 7, 13)]
    c = gc.final_check_case(small_seq, orc)
    k = np.flatnonzero(c["flips"])[:40]
    runs.append((dict(c, pts=np.ascontiguousarray(c["pts"][k]), guess=np.ascontiguousarray(c["pts"][k]), want=tuple(a[k] for a in c["want_no_err"][:2]) + (None,)),
                 GUESS | EIG))
    for c, flags in runs:
        (nxt, st, err), _ = fe.run_standalone(tmp_path, c, flags, guess=c["guess"], what=(c["win"], flags))
        fc.assert_same((nxt, st, err if c["want"][2] is not None else None), c["want"], (c["win"], flags))
