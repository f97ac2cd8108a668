"""The LK kernels with the level's choice between the 32-bit and the split iteration sums (lk.hip: lk_sums_fit, wave_sum2_f32) on
the CPU emulator, against the checker bit for bit: the 4-hop chain kernel and the two-image kernels (windows 21 and 5) on the three
160 x 120 cases of tests/lk_fit.py with 64 points.  lk.hip's emulator-only counter says which sums the iterations of a case ran
with: the low-contrast case the 32-bit ones only, the checkerboard the split ones only, the rendered crop both."""
import numpy as np
import pytest

import flow_cases as fc
import flow_emu
import lk_fit

KINDS = ("low", "checker", "synth")


@pytest.fixture(scope="module")
def lib():
    return lk_fit.emu_lib()


def _paths(kind, c, what):
    split, fit = int(c[:, 0].sum()), int(c[:, 1].sum())
    print("%s %s: iterations per level [split, 32-bit] %s" % (kind, what, c[:4].tolist()))
    assert split + fit >= 300, (kind, what, "the case iterates")
    if kind == "low":
        assert split == 0 and fit > 0, (kind, what, c.tolist())
    elif kind == "checker":
        assert fit == 0 and split > 0, (kind, what, c.tolist())
    else:
        assert split > 0 and fit > 0, (kind, what, c.tolist())


@pytest.mark.parametrize("kind", KINDS)
def test_chain_matches_checker_on_the_expected_path(lib, orc, kind):
    want_trk, want_st = lk_fit.oracle_chain(orc, kind)
    assert (want_st[3] == 1).sum() >= 32, "the checker tracks the case round the chain"
    lk_fit.emu_counts(lib, reset=True)
    trk, st = lk_fit.emu_chain(lib, lk_fit.images(kind), lk_fit.points(), 3)
    c = lk_fit.emu_counts(lib, reset=True)
    assert np.array_equal(st[0], want_st), (kind, "status", np.argwhere(st[0] != want_st)[:8].tolist())
    assert np.array_equal(fc.bits(trk[0]), fc.bits(want_trk)), (kind, "positions")
    _paths(kind, c, "chain")


@pytest.mark.parametrize("win", [21, 5])
@pytest.mark.parametrize("kind", KINDS)
def test_flow_matches_checker_on_the_expected_path(lib, orc, kind, win):
    c = lk_fit.flow_case(orc, kind, win)
    lk_fit.emu_counts(lib, reset=True)
    got, levels = flow_emu.track(lib, c)
    n = lk_fit.emu_counts(lib, reset=True)
    assert levels == c["max_level"] + 1
    fc.assert_same(got, c["want"], (kind, win))
    if win == 21:
        _paths(kind, n, "flow 21")
    else:   # 25 pixels: 25 * 4080^2 > 1.5e8 > 9 * 4080^2 -- only a window of nearly constant +-4080 fails to fit
        print("%s flow 5: iterations per level [split, 32-bit] %s" % (kind, n[:4].tolist()))
        assert n.sum() >= 100
        if kind != "checker":
            assert n[:, 0].sum() == 0
