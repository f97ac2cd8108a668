"""Inputs of the tests of lk_circular_queue_kernel (test_lk_queue_emulation.py on the CPU emulator, test_gpu_lk_queue.py on the
MI355X) and their side of the emulator harness tests/host_check/chain_emu.cpp (cq_chain).

Frames: the 96 x 88 "deep" case of lk_setup_cases.py (three levels; points inside, near and outside the image), frame f with the
case's four images rotated by f and the case's points, repeated up to 64 and rotated by f, so that no two frames of a group of
eight are alike.  What is compared is always the library (or the emulated kernel) against itself under the other split of the
work: the static lk_circular_kernel is the reference, bit for bit."""
import ctypes as C

import numpy as np

import emu_build
import lk_setup_cases as sc
from conftest import vp

W, H = sc.W, sc.H_DEEP
N = 64
_CACHE = {}


def images():
    return sc.case("deep")["imgs"]


def quads(n_frames):
    return np.array([np.roll([0, 1, 2, 3], -f) for f in range(n_frames)], np.int32)


def points(n_frames):
    """[n_frames, N, 2]: the case's points repeated to N, rotated by f"""
    key = ("points", n_frames)
    if key not in _CACHE:
        p = sc.case("deep")["pts"]
        p = np.concatenate([p] * (N // len(p) + 1))[:N]
        _CACHE[key] = np.ascontiguousarray(np.stack([np.roll(p, -f, axis=0) for f in range(n_frames)]), np.float32)
        _CACHE[key].setflags(write=False)
    return _CACHE[key]


# ---- the emulator ----------------------------------------------------------------------------------------------------------------
def emu_chain(counts, full_chain, order, first_xcd=3, surplus_div=8):
    """(trk [F, 4, N, 2], status [F, 4, N], stats) of one emulated launch over len(counts) frames; order -1: lk_circular_kernel,
    0 / 1 / 2: the queue kernel with its workgroups in dispatch order / reversed / those of XCD first_xcd first.  stats:
    (workgroups, workgroups that found every queue dry, workgroups that took another XCD's item, most draws of one workgroup,
    workgroups that found their XCD marked all dry at their first draw)"""
    cnt = np.asarray(counts, np.int32)
    nf = len(cnt)
    imgs, q, pts = np.ascontiguousarray(np.stack(images())), quads(nf), points(nf)
    trk, st = np.zeros((nf, 4, N, 2), np.float32), np.zeros((nf, 4, N), np.uint8)
    stats = np.zeros(5, np.int32)
    lib = emu_build.shared("chain_emu")   # (the library of lk_chain_cases.py, without sanitizer flags whatever the environment says)
    lib.cq_chain.restype = C.c_int
    levels = lib.cq_chain(vp(imgs), 4, W, H, 3, vp(q), nf, vp(pts), vp(cnt), N, int(full_chain), int(order), int(first_xcd), int(surplus_div),
                          vp(trk), vp(st), vp(stats))
    assert levels == sc.depth(H, 3) + 1, levels   # (negative: the counters' own checks, chain_emu.cpp)
    return trk, st, tuple(int(v) for v in stats)
