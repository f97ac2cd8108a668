"""The programs and cases of the iteration's branches (lk.hip: one loop per kind of sum, the scalar branch on iw11 = -1; vo_lkmath.h:
lk_weights_packed, blend7_cols with the caller's word on the sign), shared by test_lk_weights_on_host.py (g++: the emulator text),
test_lk_iteration_branches_emulation.py (the kernels on the CPU emulator) and test_gpu_lk_iteration_branches.py (gfx950).

The images are those of tests/lk_fit.py (low / checker / synth: every level's sums fit 32 bits, none does, both).  The points are its
64 with the first row of eight moved to corners whose fractions lie where iw00 = 16383 and iw01 = iw10 = 1 leave iw11 = -1: a point
(X + 10 + f, Y + 10 + f) has the level-0 window corner (X + f, Y + f), f in 3.2e-5 .. 4.4e-5, so the level-0 template is sampled with
iw11 = -1.  A `still` case is one image four times: the search window is the template, so the deltas vanish (but for the rounding of
(x - 10) + 10 at the coarser levels) and level 0 starts within an ulp or two of the point itself -- its first iteration samples with
iw11 = -1 too, the case of the iteration that the moving cases reach only by accident."""
import ctypes as C
import os

import numpy as np

import emu_build
import lk_fit
from conftest import ROOT

SRC_DIR = os.path.join(ROOT, "tests", "host_check")
N_NEG = 8            # points that start at a corner with iw11 = -1
HOST_PAIRS = 155122  # 256^2 + 251^2 + 128^2 + 101^2 fraction pairs of lk_weights_host.cpp
_CACHE = {}


def build_host(out_dir, sanitize=False):
    exe = os.path.join(out_dir, "lk_weights_host" + ("_san" if sanitize else ""))
    emu_build.build(exe, os.path.join(SRC_DIR, "lk_weights_host.cpp"), emu_build.FLAGS + (emu_build.SAN_PROGRAM_FLAGS if sanitize else ["-O2"]))
    return exe


def weights(a, b):
    """OpenCV's four weights of the fractions (a, b), float32 in and every product rounded to float32"""
    a, b = np.float32(a), np.float32(b)
    a1, b1 = np.float32(1) - a, np.float32(1) - b
    w = [int(np.rint(np.float64(np.float32(x * y)) * 16384.0)) for x, y in ((a1, b1), (a, b1), (a1, b))]
    return w + [16384 - sum(w)]


def points():
    if "pts" not in _CACHE:
        p = np.array(lk_fit.points())
        for k in range(N_NEG):
            f = np.float32((17 + k % 7) * 2.0 ** -19)    # 3.24e-5 .. 4.39e-5 in steps of one ulp of [16, 32)
            x, y = np.float32(20 + k) + f, np.float32(27 - k) + f
            fx, fy = np.float32(x - np.float32(10)), np.float32(y - np.float32(10))   # the corner, as the kernel forms it at level 0
            assert weights(fx - np.floor(fx), fy - np.floor(fy)) == [16383, 1, 1, -1], (k, x, y)
            p[k] = (x, y)
        p.setflags(write=False)
        _CACHE["pts"] = p
    return _CACHE["pts"]


def images(kind):
    """lk_fit's three cases, and "still": the rendered crop four times"""
    if kind == "still":
        return [lk_fit.images("synth")[0]] * 4
    return lk_fit.images(kind)


def oracle_chain(orc, kind):
    """the checker's four hops over the case from points(): trk [4, n, 2], status [4, n]"""
    key = ("chain", kind)
    if key not in _CACHE:
        l0, r0, l1, r1 = images(kind)
        trk, st, p = [], [], points()
        for a, b in ((l0, r0), (r0, r1), (r1, l1), (l1, l0)):
            p, s, _ = orc.calc_optical_flow_pyr_lk(a, b, p, max_level=lk_fit.max_level())
            trk.append(p)
            st.append(s)
        trk, st = np.stack(trk), np.stack(st)
        trk.setflags(write=False)
        st.setflags(write=False)
        _CACHE[key] = (trk, st)
    return _CACHE[key]


def flow_case(orc, kind, win):
    """images l0 -> r0 of the case from points() with a win x win window: the dict tests/flow_emu.py and the device calls take"""
    key = ("flow", kind, win)
    if key not in _CACHE:
        im = images(kind)
        want = orc.calc_optical_flow_pyr_lk(im[0], im[1], points(), win=win, max_level=lk_fit.max_level())
        for a in want:
            a.setflags(write=False)
        _CACHE[key] = dict(prev=im[0], next=im[1], pts=points(), win=win, lk_max_level=3, max_level=lk_fit.max_level(), want=want)
    return _CACHE[key]


def emu_lib():
    """liblk_branches_emu.so (tests/host_check/lk_branches_emu.cpp): lk_fit_emu.cpp and the counter of iterations with iw11 = -1"""
    lib = emu_build.shared("lk_branches_emu")
    lib.fe_track.restype = C.c_int
    lib.lf_chain.restype = C.c_int
    lib.lb_neg_iterations.restype = C.c_longlong
    return lib
