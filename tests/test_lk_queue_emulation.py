"""lk_circular_queue_kernel against lk_circular_kernel on the CPU emulator (tests/host_check/chain_emu.cpp: cq_chain): 17 frames of
the 96 x 88 "deep" case -- two groups of eight and a partial third -- with 0, 1, 5, 64, ... points, the queue kernel's workgroups
run in dispatch order, in reverse and with one XCD's workgroups before all others.  Tracks and status of all four hops, rows a
frame does not track included (they keep the fill), equal bit for bit in the default mode and with full_chain."""
import numpy as np
import pytest

import lk_queue_cases as qc

# frame f tracks COUNTS[f] points: an empty frame, single points, the longest list in one XCD's frames, a partial last group
COUNTS = (0, 1, 5, 64, 2, 3, 1, 7, 6, 0, 1, 5, 2, 3, 1, 7, 5)
ORDERS = {"dispatch": 0, "reverse": 1, "one-xcd-first": 2}
_REF = {}


def _static(full_chain):
    if full_chain not in _REF:
        trk, st, _ = qc.emu_chain(COUNTS, full_chain, -1)
        for a in (trk, st):
            a.setflags(write=False)
        _REF[full_chain] = (trk, st)
    return _REF[full_chain]


def test_static_launch_tracks_and_loses_points():
    """the reference side: every frame's rows written, rows beyond its count untouched, live and lost points, and the default
    mode retires features the full chain tracks on"""
    trk, st = _static(1)
    trk0, st0 = _static(0)
    for f, c in enumerate(COUNTS):
        assert (st[f][:, :c] <= 1).all() and (st[f][:, c:] == 0xA5).all() and (trk[f][:, c:] == (123456.0, -7.0)).all()
    big = COUNTS.index(64)
    assert (st[big][3] == 1).sum() >= 20 and (st[big][0] == 0).sum() >= 3
    assert (trk0[big][1:] == -1.0).any() and not np.array_equal(trk0, trk)


@pytest.mark.parametrize("full_chain", [0, 1], ids=["default", "full_chain"])
@pytest.mark.parametrize("order", sorted(ORDERS))
def test_queue_kernel_equals_static_kernel(order, full_chain):
    want_trk, want_st = _static(full_chain)
    trk, st, (blocks, dry, stolen, draws, marked) = qc.emu_chain(COUNTS, full_chain, ORDERS[order])
    groups, ppp = 3, max(COUNTS)
    items, surplus = groups * ppp, (groups * ppp + 7) // 8
    assert blocks == 8 * (items + surplus)
    assert dry == 8 * surplus                      # every ticket below `items` was taken by exactly as many workgroups
    assert draws == 8                              # a workgroup that finds every queue dry draws once per queue, and no more
    # ... and is the only one of its XCD that does: the others stop at their first draw (an XCD whose surplus all stole has none)
    assert dry - 8 <= marked <= dry - 1 and (order == "one-xcd-first" or marked == dry - 8)
    if order == "one-xcd-first":                   # its surplus workgroups took the first tickets of the next XCD's queue, and so on
        assert stolen >= surplus
    if order == "dispatch":
        assert stolen == 0
    assert np.array_equal(st, want_st), np.argwhere(st != want_st)[:8].tolist()
    assert np.array_equal(trk.view(np.uint32), want_trk.view(np.uint32)), np.argwhere(trk.view(np.uint32) != want_trk.view(np.uint32))[:8].tolist()
