"""The LK level entry, level set-up and cell test on the CPU: the real lk.hip through the SIMT emulator of tests/host_check (the
library tests/test_lk_iteration_paths.py builds) against the checker -- the cases of tests/lk_setup_cases.py, each crossed with its
parameter sets (lk_max_level 0 .. 4, lk_max_count 0 / 1 / 30, a sweep of lk_min_eig_threshold), full chain.  Status is compared on
every hop, positions as raw bits on every hop the checker reports alive.

What the set-up can get wrong: the start of a level (2^-level * point at the deepest one, twice the level above at every other,
untouched by a level that is refused or runs no iteration), the window test of the template and of the first cell on converted
floors (NaN, +-inf, beyond int32), the min-eigenvalue shortcut against the exact test, the reciprocal of the determinant, and
the reduction of the structure tensor."""
import ctypes as C

import numpy as np
import pytest

import lk_setup_cases as sc
from conftest import vp
from test_lk_iteration_paths import iemu  # noqa: F401  (the fixture: libkernel_emu.so without sanitizer flags, loaded once for both files)


def run_chain(lib, c, prm, variant=0):
    """the case's four hops on the emulated lk_circular_kernel (variant 2: lk_hops_kernel, hop 0 then hops 1 .. 3), full chain"""
    max_level, max_count, min_eig = prm
    imgs = np.ascontiguousarray(np.stack(c["imgs"]), np.uint8)
    pts = np.ascontiguousarray(c["pts"], np.float32)
    n = len(pts)
    lw, lh = C.c_int(0), C.c_int(0)
    trk, st = np.zeros((4, n, 2), np.float32), np.zeros((4, n), np.uint8)
    lib.ke_set_lk_pair(variant)
    try:
        levels = lib.ke_run(vp(imgs), 4, c["w"], c["h"], max_level, -1, None, None, C.byref(lw), C.byref(lh), vp(pts), n, max_count, C.c_double(0.01),
                            C.c_float(min_eig), 1, vp(trk), vp(st))
    finally:
        lib.ke_set_lk_pair(0)
    assert levels == sc.depth(c["h"], max_level) + 1
    return trk, st


def test_the_cases_take_their_paths(orc):
    seen = sc.premises(orc)
    print("solves of hop 0 by path (checker's log, numpy restatement of the set-up):", seen)


@pytest.mark.parametrize("name", sc.CASES)
def test_emulated_chain_equals_checker(iemu, orc, name):  # noqa: F811
    c = sc.case(name)
    for prm in sc.params_of(name):
        trk, st = run_chain(iemu, c, prm)
        sc.assert_chain(trk, st, sc.oracle(orc, name, prm), (name, prm))


@pytest.mark.parametrize("name", ["outside", "jump"])
def test_emulated_split_chain_equals_checker(iemu, orc, name):  # noqa: F811
    """lk_hops_kernel shares the body: hop 0, then hops 1 .. 3 from what the first launch left"""
    c = sc.case(name)
    for prm in (sc.PARAMS[1], sc.PARAMS[4]):
        trk, st = run_chain(iemu, c, prm, variant=2)
        sc.assert_chain(trk, st, sc.oracle(orc, name, prm), (name, prm, "split"))
