"""Inputs and expected answers of the context-mode tests (test_context_modes_premises.py on the CPU, test_gpu_context_modes.py on
the MI355X): the flow calls (include/vo_flow.h, vo_flow_win.h, vo_flow_flags.h) and the corner calls (vo_corners.h,
vo_corners_mask.h) in a context with rectification maps and / or a colour or interleaved input format.  Not a test file.

Nothing here is new arithmetic.  Every expected value is composed, in the order the headers state -- convert, then remap, then the
algorithm -- from code that already is the project's CPU specification:
    conversion   to_gray / colourise / FORMATS of test_gpu_ingest_formats.py (for GRAY8_X2 the other byte plane is noise)
    remap        rectify_cases.remap_ref with the maps of rectify_cases.mild_maps / make_maps
    flow         orc.calc_optical_flow_pyr_lk, flow_flags_cases.driver / plain_no_err / _bracket, flow_cases.delete_unmatch_features
    corners      corners_emu.ref_map / ref_detect, corners_mask_cases.ref_detect / ref_disc_mask
What the tests pin is the ROUTING between those: which image slot, which side's maps, which image a call reads.

Case M: 480 x 160, small_seq L0 -> L1, the 596 points small_seq["pts"][0], mild_maps.
Case S: 96 x 64, the crops cL0 -> cL1 of flow_cases.images, the point sets crop60 and lattice, make_maps(kind) for kind in S_KINDS
        (the barrel map's corners leave the image: zeros enter the tracked windows).
Expected values are computed once per session, frozen and shared."""
import numpy as np

import corners_emu as ce
import corners_mask_cases as cm
import flow_cases as fc
import flow_flags_cases as gc
import flow_win_cases as wc
from rectify_cases import make_maps, mild_maps, remap_ref
from test_gpu_ingest_formats import BGR8, BGRA8, BPP, FORMATS, GRAY8, GRAY8_X2, NAMES, RGB8, RGBA8, colourise, to_gray  # noqa: F401

S_KINDS = ("all_ab", "barrel", "edges")
# the route under test and the three wrong ones a slip gives: (side of prev's maps, side of next's maps), None = not remapped
ROUTES = {"left": (0, 0), "next_right": (0, 1), "both_right": (1, 1), "none": (None, None)}
WRONG_ROUTES = ("next_right", "both_right", "none")
BATCH_PAIRS = [(0, 2), (0, 1), (1, 3), (3, 2)]          # over the table L0, R0, L1, R1 (even index = left maps, odd = right)
CORN = dict(max_corners=0, quality_level=0.01, min_distance=5.0)
_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def frozen(a):
    a.setflags(write=False)
    return a


# ---- images, maps, points ---------------------------------------------------------------------------------------------------------
def m_maps(small_world):
    """((mx_l, my_l), (mx_r, my_r)) of case M"""
    return _once("maps-M", lambda: mild_maps(small_world.proj_matrices()[0], 480, 160))


def s_maps(kind):
    return _once(("maps-S", kind), lambda: (make_maps(kind, 96, 64, 0), make_maps(kind, 96, 64, 1)))


def case_m(small_seq, small_world):
    """dict(prev, next, pts, maps, sets): the raw pair of case M"""
    im = fc.images(small_seq)
    pts = fc.point_sets(small_seq)["pts596"]
    return dict(tag="M", prev=im["L0"], next=im["L1"], pts=pts, maps=m_maps(small_world), sets={"pts596": pts})


def case_s(kind, small_seq):
    im, ps = fc.images(small_seq), fc.point_sets(small_seq)
    return dict(tag="S-" + kind, prev=im["cL0"], next=im["cL1"], pts=ps["crop60"], maps=s_maps(kind),
                sets={"crop60": ps["crop60"], "lattice": ps["lattice"]})


def remapped(tag, img, maps, side):
    """remap_ref(img, *maps[side]) -- side None: the image as it is -- once per (tag, side)"""
    if side is None:
        return img
    return _once(("remap", tag, side), lambda: frozen(remap_ref(img, *maps[side])))


def routed_pair(c, route="left"):
    """the pair of case c as a synchronous flow call of a context with c's maps sees it under `route`"""
    a, b = ROUTES[route]
    return remapped(c["tag"] + "-prev", c["prev"], c["maps"], a), remapped(c["tag"] + "-next", c["next"], c["maps"], b)


def padded(a, extra=37, top=4, left=11):
    """the (h, w) or (h, w, bpp) array as a view into a larger buffer: a row stride that is not the width"""
    a = np.asarray(a)
    h, w = a.shape[:2]
    big = np.full((h + top + 5, w + left + extra) + a.shape[2:], 200, np.uint8)
    big[top:top + h, left:left + w] = a
    return big[top:top + h, left:left + w]


def random_guess(pts, seed=7, spread=6.0):
    """flow_flags_cases' random guess: the start point + uniform(-spread, spread)"""
    return (pts + np.random.default_rng(seed).uniform(-spread, spread, pts.shape)).astype(np.float32)


# ---- flow: the checker on a pair, as each entry point is specified ------------------------------------------------------------------
def depth_of(img, lk_max_level=3):
    h, w = img.shape
    return wc.depth(w, h, lk_max_level)


def flow_want(orc, key, pair, pts, win=21, guess=None, min_eigenvals=False):
    """(next, status, err or None) of the checker for one call on `pair` at the depth the library plans (flow_win_cases.depth):
    flags 0: calc_optical_flow_pyr_lk; a guess: flow_flags_cases.driver; min_eigenvals: the checker without an err vector (the
    values are bracketed by check_eig).  key: None = not remembered"""
    prev, nxt = pair
    e = depth_of(prev)

    def make():
        if guess is None and not min_eigenvals:
            return fc.freeze(orc.calc_optical_flow_pyr_lk(prev, nxt, pts, win=win, max_level=e))
        if guess is None:
            return fc.freeze(gc.plain_no_err(orc, prev, nxt, pts, win=win, max_level=e))
        return fc.freeze(gc.driver(prev, nxt, pts, guess, win=win, max_level=e, want_err=not min_eigenvals))

    return make() if key is None else _once(("flow", key, win, guess is not None, min_eigenvals), make)


def check_eig(orc, prev, pts, win, err, what=""):
    """err of a GET_MIN_EIGENVALS call against the checker, flow_flags_cases' way: a point whose level-0 template is inadmissible
    reports 0; every point the checker can verify (status 1 on (prev, prev) at level 0 with the threshold off) holds the checker's
    minimum eigenvalue bit for bit, by bracketing with its threshold.  Returns the number of verified points"""
    adm = gc.admissible(prev, pts, win)
    assert np.all(fc.bits(err[~adm]) == 0), (what, "an inadmissible level-0 template reports 0")
    ver = orc.calc_optical_flow_pyr_lk(prev, prev, pts, win=win, max_level=0, min_eig=-1.0)[1] == 1
    assert not (ver & ~adm).any()
    bad = [i for i in np.flatnonzero(ver) if not gc._bracket(orc, prev, pts[i], win, err[i])]
    assert not bad, (what, "min eigenvalue differs from the checker's", bad[:8], err[bad[:8]])
    return int(ver.sum())


def rows_that_differ(a, b):
    """number of points whose position bits differ between two (next, status, err) answers"""
    return int((fc.bits(a[0]) != fc.bits(b[0])).any(1).sum())


def assert_feature_tracking(r, pts, want, what=""):
    """voflow_feature_tracking's dict against deleteUnmatchFeatures on the checker's answer `want`"""
    nxt, st, err = want
    w0, w1, wst, wkeep = fc.delete_unmatch_features(pts, nxt, st)
    assert r["n_out"] == len(wkeep) and np.array_equal(r["keep_idx"], wkeep) and np.array_equal(r["status"], wst), what
    assert np.array_equal(fc.bits(r["points0"]), fc.bits(w0)) and np.array_equal(fc.bits(r["points1"]), fc.bits(w1)), what
    assert np.array_equal(fc.bits(r["err"]), fc.bits(err)), (what, "err is not compacted")


# ---- the image table of the throughput mode -----------------------------------------------------------------------------------------
def table_raw(small_seq):
    L, R = small_seq["L"], small_seq["R"]
    return [L[0], R[0], L[1], R[1]]


def table_rect(small_seq, small_world):
    """the table as a context with case M's maps holds it: image i through the maps of side i & 1"""
    maps = m_maps(small_world)
    return [remapped("table-%d" % i, img, maps, i & 1) for i, img in enumerate(table_raw(small_seq))]


# ---- colour and interleaved inputs --------------------------------------------------------------------------------------------------
def encode(gray, fmt, seed, plane=0):
    """(what a context of format fmt is handed, the gray image the header says it becomes, the gray image a WRONG reading gives).
    Colour: colourise -- channels that differ; the wrong reading exchanges the first and third channel.  GRAY8_X2: byte plane
    `plane` of a two-byte interleave whose other plane is noise; the wrong reading is that other plane"""
    if fmt == GRAY8:
        return gray, gray, None
    if fmt == GRAY8_X2:
        noise = np.random.default_rng(1000 + seed).integers(0, 256, gray.shape, dtype=np.uint8)
        frame = np.ascontiguousarray(np.stack([gray, noise] if plane == 0 else [noise, gray], axis=-1))
        return frame[..., plane], frozen(frame[..., plane].copy()), noise
    c = colourise(gray, fmt, seed)
    sw = c.copy()
    sw[..., 0], sw[..., 2] = c[..., 2], c[..., 0]
    return c, frozen(to_gray(c, fmt)), to_gray(sw, fmt)


def colour_pair(c, fmt, route="left"):
    """(prev array, next array, the gray pair after conversion and `route`) of case c in format fmt; next rides the second byte
    plane of its own buffer in GRAY8_X2"""
    def make():
        a, ga, _ = encode(c["prev"], fmt, 61)
        b, gb, _ = encode(c["next"], fmt, 62, plane=1)
        sa, sb = ROUTES[route]
        tag = "%s-%s" % (c["tag"], NAMES[fmt])
        return a, b, (remapped(tag + "-prev", ga, c["maps"], sa), remapped(tag + "-next", gb, c["maps"], sb))
    return _once(("colour", c["tag"], fmt, route), make)


# ---- corners ------------------------------------------------------------------------------------------------------------------------
def corn_want(key, img, mask=None, max_corners=0):
    """the corner list of the detector's reference with the parameters CORN (corners_emu.ref_detect; under a mask
    corners_mask_cases.ref_detect)"""
    def make():
        if mask is None:
            return frozen(ce.ref_detect(img, max_corners, CORN["quality_level"], CORN["min_distance"])[0])
        return frozen(cm.ref_detect(img, mask, max_corners, CORN["quality_level"], CORN["min_distance"])[0])
    return make() if key is None else _once(("corn", key, max_corners), make)


def map_want(key, img):
    return _once(("eigmap", key), lambda: frozen(ce.ref_map(img)))


def same_corners(got, want, what=""):
    assert got.shape == want.shape and np.array_equal(fc.bits(got), fc.bits(want)), (what, len(got), len(want))


def same_map(got, want, what=""):
    assert got.shape == want.shape and np.array_equal(fc.bits(got), fc.bits(want)), (what, int((fc.bits(got) != fc.bits(want)).sum()))


def corner_masks(w, h):
    """the masks of the corner tests: a checker of 4 x 4 cells (a remapped copy of it differs nearly everywhere) and the left half"""
    return {"checker": cm.checker(w, h), "left_half": cm.left_half(w, h)}
