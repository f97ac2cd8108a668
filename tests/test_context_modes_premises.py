"""The premises of test_gpu_context_modes.py, on the CPU with the checker alone: no comparison of that file can pass vacuously, and
none can pass with the wrong side's maps, the wrong image or the wrong channel order.  Each expected answer (tests/context_modes_cases.py)
tracks enough points, loses some, and differs in bits from what every wrong route would give.  The floors are the issue's; the
figures beside them were taken with the checker when the tests were written."""
import numpy as np
import pytest

import context_modes_cases as cc
import flow_cases as fc


# ---- case M: 480 x 160, mild maps ------------------------------------------------------------------------------------------------
def test_m_expected_answer_tracks_and_loses(orc, small_seq, small_world):
    c = cc.case_m(small_seq, small_world)
    nxt, st, err = cc.flow_want(orc, "M-left-pts596", cc.routed_pair(c), c["pts"])
    assert len(st) == 596 and cc.depth_of(c["prev"]) == 2
    assert (st == 1).sum() >= 500 and (st == 0).sum() >= 20, ((st == 1).sum(), (st == 0).sum())   # 553 tracked, 43 lost
    assert np.all(err[st == 0] == 0) and np.all(err[st == 1] > 0)


@pytest.mark.parametrize("route", cc.WRONG_ROUTES)
def test_m_every_wrong_route_gives_other_bits(orc, small_seq, small_world, route):
    """prev left / next RIGHT (k forced to 0), both RIGHT, no remap at all: 595, 596 and 595 of 596 rows differ"""
    c = cc.case_m(small_seq, small_world)
    want = cc.flow_want(orc, "M-left-pts596", cc.routed_pair(c), c["pts"])
    wrong = cc.flow_want(orc, "M-" + route, cc.routed_pair(c, route), c["pts"])
    assert cc.rows_that_differ(want, wrong) >= 590, cc.rows_that_differ(want, wrong)


@pytest.mark.parametrize("win", [5, 13])
def test_m_windows_track(orc, small_seq, small_world, win):
    """510 (5 x 5) and 531 (13 x 13) of 596 at the depth the library plans for 480 x 160 (E = 2); and the window matters: the
    21 x 21 answer differs nearly everywhere"""
    c = cc.case_m(small_seq, small_world)
    want = cc.flow_want(orc, "M-left-pts596", cc.routed_pair(c), c["pts"], win=win)
    assert (want[1] == 1).sum() >= 450, (want[1] == 1).sum()
    assert cc.rows_that_differ(want, cc.flow_want(orc, "M-left-pts596", cc.routed_pair(c), c["pts"])) >= 500


def test_m_flags_matter(orc, small_seq, small_world):
    """a guess-ignoring route, or one that keeps the final in-bounds check under GET_MIN_EIGENVALS, gives other bits"""
    c = cc.case_m(small_seq, small_world)
    pair, pts = cc.routed_pair(c), c["pts"]
    plain = cc.flow_want(orc, "M-left-pts596", pair, pts)
    guessed = cc.flow_want(orc, "M-left-pts596", pair, pts, guess=cc.random_guess(pts))
    assert cc.rows_that_differ(plain, guessed) >= 500 and (guessed[1] == 1).sum() >= 400
    wrong_side = cc.flow_want(orc, "M-next_right", cc.routed_pair(c, "next_right"), pts, guess=cc.random_guess(pts))
    assert cc.rows_that_differ(guessed, wrong_side) >= 500


# ---- case S: 96 x 64, the maps of the rectification tests ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", cc.S_KINDS)
def test_s_crop60_tracks_and_differs_from_the_wrong_routes(orc, small_seq, kind):
    """crop60 tracks 58 / 60 / 58 of 60 (all_ab, barrel, edges) and differs from the wrong routes in 56 to 60 rows"""
    c = cc.case_s(kind, small_seq)
    want = cc.flow_want(orc, c["tag"] + "-left-crop60", cc.routed_pair(c), c["pts"])
    assert len(want[1]) == 60 and cc.depth_of(c["prev"]) == 1 and (want[1] == 1).sum() >= 50, (want[1] == 1).sum()
    for route in ("next_right", "both_right"):
        wrong = cc.flow_want(orc, "%s-%s-crop60" % (c["tag"], route), cc.routed_pair(c, route), c["pts"])
        assert cc.rows_that_differ(want, wrong) >= 50, (route, cc.rows_that_differ(want, wrong))


@pytest.mark.parametrize("kind", cc.S_KINDS)
def test_s_lattice_has_both_statuses(orc, small_seq, kind):
    c = cc.case_s(kind, small_seq)
    pts = c["sets"]["lattice"]
    nxt, st, err = cc.flow_want(orc, c["tag"] + "-left-lattice", cc.routed_pair(c), pts)
    assert (st == 1).sum() >= 20 and (st == 0).sum() >= 20, ((st == 1).sum(), (st == 0).sum())


def test_s_barrel_brings_zeros_into_the_windows(small_seq):
    c = cc.case_s("barrel", small_seq)
    prev, nxt = cc.routed_pair(c)
    assert (prev[:8, :8] == 0).all() and (nxt[:8, :8] == 0).all() and prev[32:, 48:].any()
    x, y = c["pts"][:, 0], c["pts"][:, 1]
    assert ((x < 20) & (y < 20)).sum() >= 1, "a tracked window reaches the zeros"


# ---- the throughput mode's table ---------------------------------------------------------------------------------------------------
def test_table_pairs_track_by_parity(orc, small_seq, small_world):
    """every pair of the batch test tracks under its parity maps, and differs from the all-left reading wherever a right image
    takes part"""
    pts = fc.point_sets(small_seq)["pts596"]
    rect, raw, maps = cc.table_rect(small_seq, small_world), cc.table_raw(small_seq), cc.m_maps(small_world)
    for f, (a, b) in enumerate(cc.BATCH_PAIRS):
        want = cc.flow_want(orc, "table-%d" % f, (rect[a], rect[b]), pts)
        assert (want[1] == 1).sum() >= 300, (f, (want[1] == 1).sum())
        if (a | b) & 1:
            left = (cc.remapped("table-left-%d" % a, raw[a], maps, 0), cc.remapped("table-left-%d" % b, raw[b], maps, 0))
            assert cc.rows_that_differ(want, cc.flow_want(orc, None, left, pts)) >= 500, f


# ---- corners on L1 of M --------------------------------------------------------------------------------------------------------------
def test_corners_of_the_raw_and_the_remapped_image_differ(small_seq, small_world):
    """ref_detect finds 1148 corners on the raw image and 1049 on the left-remapped one; lists and quality maps differ"""
    c = cc.case_m(small_seq, small_world)
    raw, rect = c["next"], cc.routed_pair(c)[1]
    a, b = cc.corn_want("M-L1-raw", raw), cc.corn_want("M-L1-left", rect)
    assert len(a) >= 500 and len(b) >= 500 and len(a) != len(b), (len(a), len(b))
    assert not np.array_equal(a[:len(b)], b[:len(a)])
    ma, mb = cc.map_want("M-L1-raw", raw), cc.map_want("M-L1-left", rect)
    assert (fc.bits(ma) != fc.bits(mb)).mean() > 0.9
    right = cc.remapped("M-next", raw, c["maps"], 1)
    assert not np.array_equal(cc.corn_want("M-L1-right", right)[:50], b[:50]), "the right maps give other corners"


def test_a_remapped_mask_would_differ(small_seq, small_world):
    """the masks are never rectified: under a mask that went through the maps the reference finds other corners"""
    c = cc.case_m(small_seq, small_world)
    rect = cc.routed_pair(c)[1]
    for name, mask in cc.corner_masks(480, 160).items():
        moved = cc.remapped("mask-" + name, mask, c["maps"], 0)
        assert (moved != mask).any(), name
        a, b = cc.corn_want("M-L1-left-" + name, rect, mask), cc.corn_want(None, rect, moved)
        assert len(a) >= 100 and (len(a) != len(b) or not np.array_equal(a, b)), name
        assert not np.array_equal(a, cc.corn_want("M-L1-left", rect)[:len(a)]), "the mask matters"


# ---- colour and interleaved formats ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", cc.FORMATS, ids=lambda f: cc.NAMES[f])
def test_channel_order_matters(orc, small_seq, small_world, fmt):
    """the image differs from its reading with the first and third channel exchanged (GRAY8_X2: from the other byte plane), and
    the checker's tracks on the two gray pairs differ in at least half the rows (measured: all 596, every format)"""
    c = cc.case_m(small_seq, small_world)
    pa, ga, wa = cc.encode(c["prev"], fmt, 61)
    pb, gb, wb = cc.encode(c["next"], fmt, 62, plane=1)
    assert pa.shape[:2] == (160, 480) and (pa.ndim == 2) == (fmt == cc.GRAY8_X2)
    assert (ga != wa).mean() > 0.5 and (gb != wb).mean() > 0.5, ((ga != wa).mean(), (gb != wb).mean())
    assert (ga != c["prev"]).mean() > 0.5 or fmt == cc.GRAY8_X2, "the conversion is not the identity on the source image"
    right = cc.flow_want(orc, None, (ga, gb), c["pts"])
    wrong = cc.flow_want(orc, None, (wa, wb), c["pts"])
    assert (right[1] == 1).sum() >= 450, (right[1] == 1).sum()
    assert cc.rows_that_differ(right, wrong) >= 298, cc.rows_that_differ(right, wrong)


def test_colour_with_maps_differs_from_colour_alone(orc, small_seq, small_world):
    """convert, THEN remap: the BGR8 answer under the left maps is neither the unrectified one nor the one of the right maps"""
    c = cc.case_m(small_seq, small_world)
    want = cc.flow_want(orc, "M-bgr8-left", cc.colour_pair(c, cc.BGR8)[2], c["pts"])
    assert (want[1] == 1).sum() >= 450
    for route in ("none", "next_right"):
        assert cc.rows_that_differ(want, cc.flow_want(orc, None, cc.colour_pair(c, cc.BGR8, route)[2], c["pts"])) >= 500, route
