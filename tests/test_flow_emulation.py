"""The two-image tracker's kernels executed on the CPU through the coroutine SIMT emulator (tests/host_check/hip_emu.h +
flow_emu.cpp, run through tests/flow_emu.py): pyr_pass_kernel over the two images, lk_flow_kernel (visual_odom_amd/csrc/lk.hip: one
hop + the err epilogue) and flow_compact_kernel (post.hip: deleteUnmatchFeatures), from the product sources.  Positions, status
and err are compared BIT FOR BIT with the checker's calcOpticalFlowPyrLK (accum_mode 0), every point; the compaction with the
python restatement of feature.cpp:20-37 applied to the checker's outputs.  tests/flow_cases.py holds the cases and asserts, on the
checker's side, that each comparison sees both statuses, tracked points that left the image, and the zero-err rule.

The sanitizer tier is the same harness as a STAND-ALONE program (flow_emu.run_standalone).  Unit test of device code, not a
product path."""
import numpy as np
import pytest

import flow_cases as fc
import flow_emu as fe
from flow_emu import compact as fe_compact


@pytest.fixture(scope="module")
def femu():
    return fe.load()


def fe_track(lib, prev, nxt, pts, max_level=3, want_err=True, n_frames=1, frame=0):
    """the 21 x 21 window, no flags: lk_flow_kernel; the outputs of frame `frame` of the n_frames copies of the pair"""
    c = dict(prev=prev, next=nxt, pts=pts, win=21, lk_max_level=max_level)
    return fe.track(lib, c, want_err=want_err, n_frames=n_frames, frame=frame)[0]


@pytest.mark.parametrize("name", list(fc.CASES))
def test_flow_kernel_matches_checker(femu, orc, small_seq, name):
    c = fc.case(name, small_seq, orc)
    fc.assert_not_vacuous(name, c)
    got = fe_track(femu, c["prev"], c["next"], c["pts"], max_level=c["max_level"])
    fc.assert_same(got, c["want"], name)


def test_flow_kernel_without_err_gives_the_same_track(femu, orc, small_seq):
    """err not requested (a null pointer to the kernel): positions and status are those of the call with err"""
    c = fc.case("crop", small_seq, orc)
    got = fe_track(femu, c["prev"], c["next"], c["pts"], want_err=False)
    fc.assert_same(got, c["want"], "no err")


def test_flow_kernel_frames_of_one_launch(femu, orc, small_seq):
    """the same pair as frames 0 .. 8 of one launch (the frame -> XCD numbering, groups of 8 and a tail): frames 3 and 8"""
    c = fc.case("crop", small_seq, orc)
    k = 13   # (points are independent of each other: the first 13 of the case, not a multiple of the 2 / 1 parts per frame)
    for n_frames, frame in ((5, 3), (9, 8)):
        got = fe_track(femu, c["prev"], c["next"], c["pts"][:k], n_frames=n_frames, frame=frame)
        fc.assert_same(got, tuple(a[:k] for a in c["want"]), (n_frames, frame))


@pytest.mark.parametrize("seed", range(20))
def test_flow_kernel_random_crops(femu, orc, small_seq, seed):
    c = fc.random_case(seed, small_seq, orc)
    got = fe_track(femu, c["prev"], c["next"], c["pts"], max_level=c["max_level"])
    fc.assert_same(got, c["want"], seed)


def test_random_crops_are_not_vacuous(orc, small_seq):
    st = np.concatenate([fc.random_case(s, small_seq, orc)["want"][1] for s in range(20)])
    nx = np.concatenate([fc.random_case(s, small_seq, orc)["want"][0] for s in range(20)])
    assert (st == 1).sum() >= 200 and (st == 0).sum() >= 200 and ((st == 1) & ((nx < 0).any(1))).sum() >= 1
    assert {0, 1} <= {len(fc.random_case(s, small_seq, orc)["pts"]) for s in range(20)}


@pytest.mark.parametrize("name", ["L0-L1", "L0-R0", "crop", "lattice", "flat"])
@pytest.mark.parametrize("threads", [64, 256, 1024])
def test_compaction_matches_delete_unmatch_features(femu, orc, small_seq, name, threads):
    c = fc.case(name, small_seq, orc)
    nxt, st, _ = c["want"]
    w0, w1, wst, wkeep = fc.delete_unmatch_features(c["pts"], nxt, st)
    if name in ("L0-L1", "L0-R0"):
        assert 0 < len(wkeep) < (st == 1).sum() < len(st), "the rewritten status differs from LK's, and something is dropped"
    o0, o1, gst, idx, k = fe_compact(femu, c["pts"], nxt, st, threads)
    assert k == len(wkeep) and np.array_equal(idx, wkeep) and np.array_equal(gst, wst)
    assert np.array_equal(fc.bits(o0), fc.bits(w0)) and np.array_equal(fc.bits(o1), fc.bits(w1))


def test_compaction_of_nothing_and_of_nan(femu):
    o0, o1, st, idx, k = fe_compact(femu, np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32), np.zeros(0, np.uint8), 64)
    assert k == 0
    # a NaN coordinate is not "< 0": the reference keeps such a point if LK says it tracked
    nxt = np.array([[np.nan, 3], [-0.0, 2], [-1e-30, 2], [5, np.inf]], np.float32)
    st = np.array([1, 1, 1, 0], np.uint8)
    pts = np.arange(8, dtype=np.float32).reshape(4, 2)
    w0, w1, wst, wkeep = fc.delete_unmatch_features(pts, nxt, st)
    o0, o1, gst, idx, k = fe_compact(femu, pts, nxt, st, 64)
    assert list(wkeep) == [0, 1] and np.array_equal(idx, wkeep) and np.array_equal(gst, wst) and np.array_equal(fc.bits(o1), fc.bits(w1))


@pytest.mark.sanitize
def test_flow_kernels_standalone_under_sanitizers(tmp_path, orc, small_seq):
    """ASan + UBSan over the kernel sources in a program of its own: exactly sized pyramid levels, no report, the same bits"""
    for name in ("crop", "lattice"):
        c = fc.case(name, small_seq, orc)
        got, (k, st2, idx) = fe.run_standalone(tmp_path, dict(c, win=21, lk_max_level=c["max_level"]), what=name)
        fc.assert_same(got, c["want"], name)
        _, _, wst, wkeep = fc.delete_unmatch_features(c["pts"], *c["want"][:2])
        assert k == len(wkeep) and np.array_equal(idx, wkeep) and np.array_equal(st2, wst)
