"""The windowed two-image tracker's kernels (visual_odom_amd/csrc/lk.hip: lk_flow_win_kernel<W>, W odd in 5 .. 19) executed on the
CPU through the coroutine SIMT emulator (tests/host_check/hip_emu.h + flow_emu.cpp, run through tests/flow_emu.py), from the
product source.  Positions, status and err are compared BIT FOR BIT, every point, with the checker's
calcOpticalFlowPyrLK(win=W, max_level=E) (accum_mode 0), E being the depth the library plans (tests/flow_win_cases.py, which also
holds the premises every comparison asserts first).

The sanitizer tier is the same harness as a STAND-ALONE program (flow_emu.run_standalone).  Unit test of device code, not a
product path."""
import ctypes as C

import numpy as np
import pytest

import flow_cases as fc
import flow_emu as fe
import flow_win_cases as wc
from conftest import vp


@pytest.fixture(scope="module")
def wemu():
    return fe.load()


def fw_track(lib, c, want_err=True, n_frames=1, frame=0, n=None):
    """the case's pair through the emulated kernel of its window, with the context's lk_max_level (the harness plans the levels)"""
    got, levels = fe.track(lib, c, want_err=want_err, n_frames=n_frames, frame=frame, n=n)
    assert levels == c["max_level"] + 1, "the harness plans the levels the depth rule says"
    return got


@pytest.mark.parametrize("name", ["crop", "lattice", "flat"])
@pytest.mark.parametrize("win", wc.WINDOWS)
def test_win_kernel_matches_checker(wemu, orc, small_seq, win, name):
    c = wc.case(name, win, small_seq, orc)
    wc.premises(name, c)
    fc.assert_same(fw_track(wemu, c), c["want"], (name, win))


@pytest.mark.parametrize("win", [5, 7, 13, 15, 19])
def test_win_kernel_on_the_full_frame(wemu, orc, small_seq, win):
    c = wc.case("L0-L1", win, small_seq, orc)
    wc.premises("L0-L1", c)
    fc.assert_same(fw_track(wemu, c), c["want"], ("L0-L1", win))


@pytest.mark.parametrize("win", [9])
def test_win_kernel_single_level(wemu, orc, small_seq, win):
    """lk_max_level 0: level 0 is the first and the last level"""
    c = wc.case("L0-L1-level0", win, small_seq, orc)
    wc.premises("L0-L1-level0", c)
    fc.assert_same(fw_track(wemu, c), c["want"], ("level0", win))


def test_win_kernel_without_err_gives_the_same_track(wemu, orc, small_seq):
    c = wc.case("crop", 11, small_seq, orc)
    fc.assert_same(fw_track(wemu, c, want_err=False), c["want"], "no err")


def test_win_kernel_frames_of_one_launch(wemu, orc, small_seq):
    """the same pair as frames of one launch (the frame -> XCD numbering, groups of 8 and a tail): frames 3 of 5 and 8 of 9"""
    c = wc.case("crop", 9, small_seq, orc)
    k = 13
    for n_frames, frame in ((5, 3), (9, 8)):
        got = fw_track(wemu, c, n_frames=n_frames, frame=frame, n=k)
        fc.assert_same(got, tuple(a[:k] for a in c["want"]), (n_frames, frame))


def test_window_21_is_the_flow_kernel(wemu, orc, small_seq):
    """the launcher's route for 21: flow_cases' crop (max_level 3 -> two levels on 96 x 64)"""
    f = fc.case("crop", small_seq, orc)
    c = dict(prev=f["prev"], next=f["next"], pts=f["pts"], win=21, lk_max_level=3, max_level=1)
    fc.assert_same(fw_track(wemu, c), f["want"], "win 21")


def test_windows_without_a_kernel_are_refused(wemu):
    img = np.zeros((64, 96), np.uint8)
    pts = np.zeros((1, 2), np.float32)
    out, st = np.zeros((1, 2), np.float32), np.zeros(1, np.uint8)
    for win in (-1, 0, 3, 4, 6, 20, 22, 23, 31):
        assert wemu.fe_track(vp(img), vp(img), 96, 64, 3, vp(pts), 1, win, 0, 30, C.c_double(0.01), C.c_float(1e-3), vp(out), vp(st), None, 1, None) == -1


@pytest.mark.parametrize("seed", range(wc.N_RANDOM))
def test_win_kernel_random_crops(wemu, orc, small_seq, seed):
    c = wc.random_case(seed, small_seq, orc)
    fc.assert_same(fw_track(wemu, c), c["want"], (seed, c["win"]))


def test_random_crops_are_not_vacuous(orc, small_seq):
    cs = [wc.random_case(s, small_seq, orc) for s in range(wc.N_RANDOM)]
    st = np.concatenate([c["want"][1] for c in cs])
    assert (st == 1).sum() >= 100 and (st == 0).sum() >= 100
    assert {c["win"] for c in cs} == set(wc.WINDOWS), "every window is drawn"


@pytest.mark.parametrize("win", wc.WINDOWS)
def test_depth_and_window_premises(orc, small_seq, win):
    """what makes a wrong depth or an ignored window fail: on L0-L1 the checker at OpenCV's own depth (3) differs from the checker
    at E = 2 in at least 500 points, and the expected positions differ from the 21 x 21 ones in at least 590 of 596"""
    assert wc.depth(480, 160, 3) == 2 and wc.depth(96, 64, 3) == 1 and [wc.depth(1241, 376, m) for m in range(5)] == [0, 1, 2, 3, 4]
    assert wc.depth_premise(win, small_seq, orc) >= 500
    assert wc.window_premise(win, small_seq, orc) >= 590


@pytest.mark.parametrize("win", wc.WINDOWS)
def test_stereo_pair_premises_for_every_window(orc, small_seq, win):
    """L0-R0 (the pair the compaction tests use): the floors, and a tracked point with a negative coordinate, for every window"""
    wc.premises("L0-R0", wc.case("L0-R0", win, small_seq, orc))


def test_depth_premise_at_21(orc, small_seq):
    """at 21 OpenCV stops where the library stops: asking for level 3 gives the bits of level 2"""
    assert wc.depth_premise(21, small_seq, orc) == 0


@pytest.mark.sanitize
def test_win_kernels_standalone_under_sanitizers(tmp_path, orc, small_seq):
    """ASan + UBSan over the kernel source in a program of its own: exactly sized pyramid levels, no report, the same bits"""
    for win in (5, 13, 15, 19):
        for name in ("crop", "lattice"):
            c = wc.case(name, win, small_seq, orc)
            got, _ = fe.run_standalone(tmp_path, c, what=(name, win))
            fc.assert_same(got, c["want"], (name, win))
