"""lk.hip's kernels on the CPU emulator at the smallest shapes where the search tile's fill and clamping matter
(tests/lk_chain_cases.py): the 4-hop chain in batches of 1, 3 and 9 frames against the checker, the split chain against the one
launch, and the two-image calls of four windows with err and with each flag.  tests/test_gpu_lk_tile.py repeats every case on
the MI355X; this file is what checks a change to the tile fill or to the samplers before any GPU time is spent."""
import numpy as np
import pytest

import flow_cases as fc
import flow_emu
import flow_flags_cases as gc
import lk_chain_cases as lc


@pytest.mark.parametrize("n_frames", lc.BATCHES)
@pytest.mark.parametrize("shape", lc.SHAPES, ids=lambda s: "%dx%d" % s)
def test_emulated_chain_in_batches(orc, shape, n_frames):
    lc.chain_premises(shape, lc.oracle_chain(orc, shape, 0))
    lc.assert_chain(orc, shape, lc.emu_chain(shape, n_frames), "batch of %d" % n_frames)


@pytest.mark.parametrize("shape,n_frames", [(lc.SHAPES[0], 1), (lc.SHAPES[0], 3), (lc.SHAPES[1], 1)], ids=["131x97-1", "131x97-3", "169x169-1"])
def test_emulated_split_chain_equals_one_launch(shape, n_frames):
    """lk_hops_kernel [0, 1) + [1, 4) over garbage outputs against lk_circular_kernel, in the default mode (a feature retires at its
    first rejected hop) -- every row a frame tracks, bit for bit"""
    one, st1, cnt = lc.emu_chain(shape, n_frames, full_chain=0)
    two, st2, _ = lc.emu_chain(shape, n_frames, full_chain=0, split=1)
    assert (st1[0][:, :cnt[0]] == 0).any() and (st1[0][3, :cnt[0]] == 1).any()
    for f, c in enumerate(cnt):
        assert np.array_equal(st1[f][:, :c], st2[f][:, :c]) and np.array_equal(fc.bits(one[f][:, :c]), fc.bits(two[f][:, :c])), f


def test_emulated_chain_reads_stay_inside_their_levels(tmp_path, orc):
    """the 169 x 169 frame as a stand-alone ASan + UBSan program: every level in a heap block of its own, so a tile fill beyond
    a clamped origin's rectangle is a report"""
    shape = lc.SHAPES[1]
    lc.assert_chain(orc, shape, lc.emu_chain_standalone(tmp_path, shape, 1), "stand-alone")


@pytest.mark.parametrize("win", lc.WINDOWS)
@pytest.mark.parametrize("shape", lc.SHAPES, ids=lambda s: "%dx%d" % s)
def test_emulated_two_image_calls(orc, shape, win):
    """err, USE_INITIAL_FLOW and GET_MIN_EIGENVALS of one window: the references of test_flow_win_emulation.py /
    test_flow_flags_emulation.py"""
    lib = flow_emu.load()
    c = lc.flow_case(shape, win, orc)
    assert (c["want"][1] == 1).sum() >= 15 and (c["want"][1] == 0).sum() >= 15 and (c["want"][2] > 0).any()
    got, levels = flow_emu.track(lib, c)
    assert levels == c["max_level"] + 1
    fc.assert_same(got, c["want"], (shape, win, "err"))
    g = lc.guess_case(shape, win, orc)
    fc.assert_same(flow_emu.track(lib, g, flags=gc.FLAG_GUESS, guess=g["guess"])[0], g["want"], (shape, win, "guess"))
    s = lc.eig_set(shape, win, orc)
    e = dict(prev=s["img"], next=s["img"], pts=s["pts"], win=win, lk_max_level=0)
    gc.check_min_eigenvals(orc, s, flow_emu.track(lib, e, flags=gc.FLAG_EIG)[0], (shape, win, "min eigenvalue"))


@pytest.mark.parametrize("win", [w for w in lc.ALL_WINDOWS if w not in lc.WINDOWS])
def test_emulated_flag_kernels_of_the_other_windows(orc, win):
    """USE_INITIAL_FLOW and GET_MIN_EIGENVALS of the windows the test above leaves out, at 131 x 97: with it, every case of
    test_gpu_lk_tile.py::test_flag_kernels_of_every_window runs here too, so a failure on the device alone is the device's"""
    shape, lib = lc.SHAPES[0], flow_emu.load()
    g, s, e = lc.flag_cases(shape, win, orc)
    fc.assert_same(flow_emu.track(lib, g, flags=gc.FLAG_GUESS, guess=g["guess"])[0], g["want"], (shape, win, "guess"))
    gc.check_min_eigenvals(orc, s, flow_emu.track(lib, e, flags=gc.FLAG_EIG)[0], (shape, win, "min eigenvalue"))


def test_emulated_two_image_batch(orc):
    """three frames of one launch with their own counts (parts of a frame's list over 4 XCDs), W = 13"""
    shape, win = lc.SHAPES[1], 13
    c = lc.flow_case(shape, win, orc)
    cnt = lc.counts(3, len(c["pts"]))
    (nxt, st, err), _ = flow_emu.track(flow_emu.load(), c, counts=cnt, frame=None)
    for f, k in enumerate(cnt):
        fc.assert_same((nxt[f][:k], st[f][:k], err[f][:k]), tuple(a[:k] for a in c["want"]), (f, k))
