"""The LK iteration with one loop per kind of sum and a scalar branch on iw11 = -1 (lk.hip, vo_lkmath.h) on the CPU emulator, against the
checker bit for bit: the 4-hop chain kernel and the two-image kernels (windows 21 and 5) on the 160 x 120 cases of tests/lk_branches.py
-- the images of tests/lk_fit.py with 64 points, eight of which start at a window corner whose weights have iw11 = -1.

lk.hip's emulator-only counters say what ran: per level, the iterations of the loop with the 32-bit sums and of the loop with the split
ones (the low-contrast case the first only, the checkerboard the second only, the rendered crop both), and the iterations that took
the out-of-line blend with iw11 = -1.  The `still` case (one image four times: the deltas vanish but for the rounding of the
coarser levels' (x - 10) + 10, so level 0 starts within an ulp or two of the point itself) makes the ITERATION take it.  On the moving
cases the template takes it at level 0 and the iteration only where a corner happens to land there; the test prints that count and
asks nothing of it (tests/test_lk_weights_on_host.py holds that case's arithmetic on 6 400 vectors)."""
import numpy as np
import pytest

import flow_cases as fc
import flow_emu
import lk_branches
import lk_fit

KINDS = ("low", "checker", "synth", "still")


@pytest.fixture(scope="module")
def lib():
    return lk_branches.emu_lib()


def _versions(kind, c, what):
    split, fit = int(c[:, 0].sum()), int(c[:, 1].sum())
    print("%s %s: iterations per level [split, 32-bit] %s" % (kind, what, c[:4].tolist()))
    assert split + fit >= (300 if kind != "still" else 64), (kind, what, "the case iterates")
    if kind == "low":
        assert split == 0 and fit > 0, (kind, what, c.tolist())
    elif kind == "checker":
        assert fit == 0 and split > 0, (kind, what, c.tolist())
    elif kind == "synth":
        assert split > 0 and fit > 0, (kind, what, c.tolist())


@pytest.mark.parametrize("kind", KINDS)
def test_chain_matches_checker_and_runs_the_versions_it_should(lib, orc, kind):
    want_trk, want_st = lk_branches.oracle_chain(orc, kind)
    assert (want_st[3] == 1).sum() >= 32, "the checker tracks the case round the chain"
    lk_fit.emu_counts(lib, reset=True)
    lib.lb_neg_iterations(1)
    trk, st = lk_fit.emu_chain(lib, lk_branches.images(kind), lk_branches.points(), 3)
    c = lk_fit.emu_counts(lib, reset=True)
    neg = lib.lb_neg_iterations(1)
    assert np.array_equal(st[0], want_st), (kind, "status", np.argwhere(st[0] != want_st)[:8].tolist())
    assert np.array_equal(fc.bits(trk[0]), fc.bits(want_trk)), (kind, "positions")
    _versions(kind, c, "chain")
    print("%s chain: %d iterations with iw11 = -1" % (kind, neg))
    if kind == "still":
        assert neg >= 1, "the iteration's out-of-line blend ran"


@pytest.mark.parametrize("win", [21, 5])
@pytest.mark.parametrize("kind", KINDS)
def test_flow_matches_checker(lib, orc, kind, win):
    c = lk_branches.flow_case(orc, kind, win)
    lk_fit.emu_counts(lib, reset=True)
    lib.lb_neg_iterations(1)
    got, levels = flow_emu.track(lib, c)
    n = lk_fit.emu_counts(lib, reset=True)
    neg = lib.lb_neg_iterations(1)
    assert levels == c["max_level"] + 1
    fc.assert_same(got, c["want"], (kind, win))
    print("%s flow %d: iterations per level [split, 32-bit] %s, %d with iw11 = -1" % (kind, win, n[:4].tolist(), neg))
    if win == 21:
        _versions(kind, n, "flow 21")
    if kind == "still" and win == 21:   # (5 x 5: printed only -- whether one of the eight small templates passes the eigenvalue test is the image's word)
        assert neg >= 1, (kind, win)
