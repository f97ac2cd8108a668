"""The two-image tracker's kernels with flags (visual_odom_amd/csrc/lk.hip: lk_flow_flags_kernel<W>, every odd W of 5 .. 21)
executed on the CPU through the coroutine SIMT emulator (tests/host_check/hip_emu.h + flow_flags_emu.cpp, over flow_emu.cpp's
harness), from the product source.  The expected side is the checker's (tests/flow_flags_cases.py): for USE_INITIAL_FLOW the
checker's own level loop started at the guess (tests/host_check/lk_flags_ref.c; its pin is the first test here), for
GET_MIN_EIGENVALS the checker without an err vector and its threshold as a bracket around every value.  Positions, status and err
are compared BIT FOR BIT, every point (NaN included), after the premises that make a guess-ignoring or epilogue-keeping kernel fail.

The library loaded into python is built WITHOUT sanitizer flags whatever the environment says.  The sanitizer tier is the same
harness as a STAND-ALONE program with its own main(), built with -fsanitize=address,undefined (runtimes linked statically) and run
as a child.  Unit test of device code, not a product path."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import flow_cases as fc
import flow_flags_cases as gc
import flow_win_cases as wc
from conftest import ROOT, vp

SRC_DIR = os.path.join(ROOT, "tests", "host_check")
CSRC = os.path.join(ROOT, "visual_odom_amd", "csrc")
OUT_DIR = os.path.join(ROOT, "tests", "_build")
DEPS = [os.path.join(SRC_DIR, f) for f in ("flow_flags_emu.cpp", "flow_emu.cpp", "hip_emu.h")] + \
       [os.path.join(CSRC, f) for f in ("lk.hip", "dev/lk_dev.hip", "pyramid.hip", "post.hip", "vo_dev.h", "vo_kernels.h", "vo_lkmath.h", "vo_isa.h", "vo_tri.h")]
CXX = ["g++", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-Wno-attributes"]
ALL_WINDOWS = wc.WINDOWS + (21,)
GUESS, EIG = gc.FLAG_GUESS, gc.FLAG_EIG


def _stale(target):
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in DEPS)


@pytest.fixture(scope="module")
def femu():
    os.makedirs(OUT_DIR, exist_ok=True)
    so = os.path.join(OUT_DIR, "libflow_flags_emu.so")
    if _stale(so):
        subprocess.check_call(CXX + ["-O2", "-fPIC", "-shared", "-o", so, os.path.join(SRC_DIR, "flow_flags_emu.cpp")])
    lib = C.CDLL(so)
    lib.ff_track.restype = C.c_int
    return lib


def ff_track(lib, c, flags, guess=None, want_err=True, counts=None, max_count=30):
    """the case's pair through the emulated kernel of its window and flags, with the context's lk_max_level; one frame, or
    len(counts) frames of one launch: (next [F, n, 2], status [F, n], err [F, n] or None), F squeezed away for one frame"""
    prev, nxt = np.ascontiguousarray(c["prev"]), np.ascontiguousarray(c["next"])
    h, w = prev.shape
    pts = np.ascontiguousarray(c["pts"], np.float32).reshape(-1, 2)
    n, nf = len(pts), 1 if counts is None else len(counts)
    io = np.zeros((nf, n, 2), np.float32)
    if guess is not None:
        io[:] = np.asarray(guess, np.float32).reshape(-1, n, 2)
    st = np.zeros((nf, n), np.uint8)
    err = np.zeros((nf, n), np.float32)
    cnt = None if counts is None else np.asarray(counts, np.int32)
    levels = lib.ff_track(vp(prev), vp(nxt), w, h, c["lk_max_level"], vp(pts), n, c["win"], flags, max_count, C.c_double(0.01), C.c_float(1e-3),
                          vp(io), vp(st), vp(err) if want_err else None, nf, None if cnt is None else vp(cnt))
    assert levels == c["max_level"] + 1, "the harness plans the levels the depth rule says"
    if counts is None:
        return io[0], st[0], (err[0] if want_err else None)
    return io, st, (err if want_err else None)


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
        assert femu.ff_track(vp(img), vp(img), 96, 64, 3, vp(pts), 1, win, flags, 30, C.c_double(0.01), C.c_float(1e-3), vp(io), vp(st), None, 1, None) == -1


@pytest.mark.sanitize
def test_flags_kernels_standalone_under_sanitizers(tmp_path, orc, small_seq):
    """ASan + UBSan over the kernel source in a program of its own: exactly sized pyramid levels, far-off starts, no report, the
    same bits"""
    out_dir = os.path.join(OUT_DIR, "san")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "flow_flags_emu_main")
    if _stale(exe):
        subprocess.check_call(CXX + ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                     "-static-libasan", "-static-libubsan", "-DFLOW_FLAGS_EMU_MAIN", "-o", exe, os.path.join(SRC_DIR, "flow_flags_emu.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    runs = [(gc.adversarial_case(win, small_seq, orc), GUESS) for win in (21, 7, 13)]
    c = gc.final_check_case(small_seq, orc)
    k = np.flatnonzero(c["flips"])[:40]
    runs.append((dict(c, pts=np.ascontiguousarray(c["pts"][k]), guess=np.ascontiguousarray(c["pts"][k]), want=tuple(a[k] for a in c["want_no_err"][:2]) + (None,)),
                 GUESS | EIG))
    for c, flags in runs:
        h, w = c["prev"].shape
        n = len(c["pts"])
        fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(fin, "wb") as f:
            f.write(np.array([w, h, c["lk_max_level"], n, c.get("max_count", 30), c["win"], flags], np.int32).tobytes())
            f.write(np.array([0.01], np.float64).tobytes() + np.array([1e-3], np.float32).tobytes())
            f.write(c["prev"].tobytes() + c["next"].tobytes() + c["pts"].tobytes() + np.ascontiguousarray(c["guess"], np.float32).tobytes())
        p = subprocess.run([exe, fin, fout], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        text = "\n".join(l for l in p.stdout.splitlines() if "doesn't fully support makecontext/swapcontext" not in l)
        assert p.returncode == 0 and "ERROR" not in text and "runtime error" not in text, ((c["win"], flags), text[-4000:])
        raw = np.fromfile(fout, np.uint8)
        nxt = raw[:8 * n].view(np.float32).reshape(n, 2)
        err = raw[8 * n:12 * n].view(np.float32)
        st = raw[12 * n:13 * n]
        fc.assert_same((nxt, st, err if c["want"][2] is not None else None), c["want"], (c["win"], flags))
