"""The two-image tracker's kernels executed on the CPU through the coroutine SIMT emulator (tests/host_check/hip_emu.h +
flow_emu.cpp): pyr_pass_kernel over the two images, lk_flow_kernel (visual_odom_amd/csrc/lk.hip: one hop + the err epilogue) and
flow_compact_kernel (post.hip: deleteUnmatchFeatures), from the product sources.  Positions, status and err are compared BIT FOR
BIT with the checker's calcOpticalFlowPyrLK (accum_mode 0), every point; the compaction with the python restatement of
feature.cpp:20-37 applied to the checker's outputs.  tests/flow_cases.py holds the cases and asserts, on the checker's side,
that each comparison sees both statuses, tracked points that left the image, and the zero-err rule.

The sanitizer tier is a STAND-ALONE program: the same harness with a main() of its own, every pyramid level in an exactly sized
heap block, built with -fsanitize=address,undefined (runtimes linked statically) and run as a child.  Nothing instrumented is
loaded into python.  Unit test of device code, not a product path."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import flow_cases as fc
from conftest import BUILD_DIR, ROOT, SAN_FLAGS, vp

SRC_DIR = os.path.join(ROOT, "tests", "host_check")
CSRC = os.path.join(ROOT, "visual_odom_amd", "csrc")
DEPS = [os.path.join(SRC_DIR, f) for f in ("flow_emu.cpp", "hip_emu.h")] + \
       [os.path.join(CSRC, f) for f in ("lk.hip", "dev/lk_dev.hip", "pyramid.hip", "post.hip", "vo_dev.h", "vo_kernels.h", "vo_lkmath.h", "vo_isa.h", "vo_tri.h")]
CXX = ["g++", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-Wno-attributes"]


def _stale(target):
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in DEPS)


@pytest.fixture(scope="module")
def femu():
    os.makedirs(BUILD_DIR, exist_ok=True)
    so = os.path.join(BUILD_DIR, "libflow_emu.so")
    if _stale(so):
        subprocess.check_call(CXX + ["-O2", "-fPIC", "-shared"] + SAN_FLAGS + ["-o", so, os.path.join(SRC_DIR, "flow_emu.cpp")])
    lib = C.CDLL(so)
    lib.fe_track.restype = C.c_int
    lib.fe_compact.restype = C.c_int
    return lib


def fe_track(lib, prev, nxt, pts, max_level=3, max_count=30, eps=0.01, min_eig=1e-3, want_err=True, n_frames=1, frame=0):
    h, w = prev.shape
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    n = len(pts)
    out = np.zeros((max(n, 1), 2), np.float32)
    st = np.zeros(max(n, 1), np.uint8)
    err = np.zeros(max(n, 1), np.float32)
    lib.fe_track(vp(np.ascontiguousarray(prev)), vp(np.ascontiguousarray(nxt)), w, h, max_level, vp(pts), n, max_count, C.c_double(eps),
                 C.c_float(min_eig), vp(out), vp(st), vp(err) if want_err else None, n_frames, frame)
    return out[:n], st[:n], (err[:n] if want_err else None)


def fe_compact(lib, pts0, nxt, status, threads):
    n = len(status)
    st = status.copy()
    o0, o1 = np.zeros((max(n, 1), 2), np.float32), np.zeros((max(n, 1), 2), np.float32)
    idx = np.full(max(n, 1), -1, np.int32)
    k = lib.fe_compact(vp(np.ascontiguousarray(pts0, np.float32)), vp(np.ascontiguousarray(nxt, np.float32)), vp(st), n, vp(o0), vp(o1), vp(idx), threads)
    return o0[:k], o1[:k], st, idx[:k], k


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
    out_dir = os.path.join(ROOT, "tests", "_build", "san")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "flow_emu_main")
    if _stale(exe):
        subprocess.check_call(CXX + ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                     "-static-libasan", "-static-libubsan", "-DFLOW_EMU_MAIN", "-o", exe, os.path.join(SRC_DIR, "flow_emu.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for name in ("crop", "lattice"):
        c = fc.case(name, small_seq, orc)
        h, w = c["prev"].shape
        n = len(c["pts"])
        fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(fin, "wb") as f:
            f.write(np.array([w, h, c["max_level"], n, 30], np.int32).tobytes())
            f.write(np.array([0.01], np.float64).tobytes() + np.array([1e-3], np.float32).tobytes())
            f.write(c["prev"].tobytes() + c["next"].tobytes() + c["pts"].tobytes())
        p = subprocess.run([exe, fin, fout], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        text = "\n".join(l for l in p.stdout.splitlines() if "doesn't fully support makecontext/swapcontext" not in l)
        assert p.returncode == 0 and "ERROR" not in text and "runtime error" not in text, text[-4000:]
        raw = np.fromfile(fout, np.uint8)
        nxt = raw[:8 * n].view(np.float32).reshape(n, 2)
        err = raw[8 * n:12 * n].view(np.float32)
        st = raw[12 * n:13 * n]
        fc.assert_same((nxt, st, err), c["want"], name)
        k = int(raw[13 * n:13 * n + 4].view(np.int32)[0])
        st2 = raw[13 * n + 4:14 * n + 4]
        idx = raw[14 * n + 4:14 * n + 4 + 4 * n].view(np.int32)[:k]
        _, _, wst, wkeep = fc.delete_unmatch_features(c["pts"], *c["want"][:2])
        assert k == len(wkeep) and np.array_equal(idx, wkeep) and np.array_equal(st2, wst)
