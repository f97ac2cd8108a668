"""Every way out of the LK Gauss-Newton iteration, on the CPU: the real lk.hip through the SIMT emulator of tests/host_check
(kernel_emu.cpp, loaded here WITHOUT sanitizer flags whatever the environment says) against the checker -- the cases of
tests/lk_iteration_cases.py, each crossed with max_count in {1, 2, 30} and epsilon in {1e-30, 0.01, 10}.  Status is compared on every
hop, positions as raw bits on every hop the checker reports alive.

The iteration is one loop with a wave-uniform "another cell" branch, unrolled by two (the previous delta is the other half's);
the window corner plus half a window is formed behind the loop, by how it was left.  What that can get wrong is a way out taken in
the wrong half, before the first iteration, or with the half step of the oscillation test in another rounding order: the sweep
takes every exit at the first, the second and a later iteration, in levels above 0 and at level 0."""
import ctypes as C

import numpy as np
import pytest

import emu_build
import lk_iteration_cases as ic
from conftest import vp


@pytest.fixture(scope="module")
def iemu():
    lib = emu_build.shared("kernel_emu")
    lib.ke_run.restype = C.c_int
    return lib


def run_chain(lib, c, max_count, eps, variant=0):
    """the case's four hops on the emulated lk_circular_kernel (variant 2: lk_hops_kernel, hop 0 then hops 1 .. 3), full chain"""
    imgs = np.ascontiguousarray(np.stack(c["imgs"]), np.uint8)
    pts = np.ascontiguousarray(c["pts"], np.float32)
    n = len(pts)
    lw, lh = C.c_int(0), C.c_int(0)
    trk, st = np.zeros((4, n, 2), np.float32), np.zeros((4, n), np.uint8)
    lib.ke_set_lk_pair(variant)
    try:
        levels = lib.ke_run(vp(imgs), 4, ic.W, ic.H, ic.MAX_LEVEL, -1, None, None, C.byref(lw), C.byref(lh), vp(pts), n, max_count, C.c_double(eps),
                            C.c_float(1e-3), 1, vp(trk), vp(st))
    finally:
        lib.ke_set_lk_pair(0)
    assert levels >= 2
    return trk, st


def test_the_sweep_takes_every_exit(orc):
    seen = ic.premises(orc)
    print("exits over the sweep (checker's logs):", seen)


@pytest.mark.parametrize("name", ic.CASES)
def test_emulated_chain_equals_checker(iemu, orc, name):
    c = ic.case(name)
    for mc in ic.MAX_COUNTS:
        for eps in ic.EPSILONS:
            trk, st = run_chain(iemu, c, mc, eps)
            ic.assert_chain(trk, st, ic.oracle(orc, name, mc, eps), (name, mc, eps))


@pytest.mark.parametrize("name", ["shift-6.2", "borders"])
def test_emulated_split_chain_equals_checker(iemu, orc, name):
    """lk_hops_kernel shares the body: hop 0, then hops 1 .. 3 from what the first launch left"""
    c = ic.case(name)
    for mc, eps in ((30, 0.01), (2, 1e-30), (30, 1e-30)):
        trk, st = run_chain(iemu, c, mc, eps, variant=2)
        ic.assert_chain(trk, st, ic.oracle(orc, name, mc, eps), (name, mc, eps, "split"))
