"""Inputs and expected results of the two-image tracker tests (test_flow_emulation.py on the CPU emulator, test_gpu_flow.py on the
MI355X): the named cases, the checker's (orc.calc_optical_flow_pyr_lk, accum_mode 0) answer for each -- computed once per session
and never modified -- the premises every comparison asserts first, and deleteUnmatchFeatures restated in python."""
import numpy as np

_CACHE = {}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def lattice(w, h, step=6.5):
    """start points from -30 to w + 40 and -30 to h + 40: the admissibility window (-21 - 10 .. ) and the final bounds check"""
    xs = np.arange(-30.0, w + 40.0 + 1e-3, step, dtype=np.float32)
    ys = np.arange(-30.0, h + 40.0 + 1e-3, step, dtype=np.float32)
    return np.stack(np.meshgrid(xs, ys), -1).reshape(-1, 2).astype(np.float32)


def images(small_seq):
    """name -> image: the small_seq frames, the 96 x 64 crops and a flat image"""
    L, R = small_seq["L"], small_seq["R"]
    im = {"L0": L[0], "L1": L[1], "L2": L[2], "R0": R[0], "R1": R[1]}
    im["cL0"] = np.ascontiguousarray(L[0][:64, :96])
    im["cL1"] = np.ascontiguousarray(L[1][:64, :96])
    im["flat"] = np.full((64, 96), 117, np.uint8)
    return im


def point_sets(small_seq):
    from visual_odom_amd import synth
    im = images(small_seq)
    pts596 = np.ascontiguousarray(small_seq["pts"][0], np.float32)
    crop60 = np.ascontiguousarray(synth.select_keypoints(im["cL0"], bucket=8, per_bucket=1), np.float32)
    rng = np.random.default_rng(50)
    flat50 = np.stack([rng.uniform(5, 90, 50), rng.uniform(5, 58, 50)], -1).astype(np.float32)
    return {"pts596": pts596, "crop60": crop60, "flat50": flat50, "lattice": lattice(96, 64)}


# name -> (prev image, next image, point set, max_level)
CASES = {
    "L0-L1": ("L0", "L1", "pts596", 3),
    "L0-R0": ("L0", "R0", "pts596", 3),
    "L0-L0": ("L0", "L0", "pts596", 3),
    "L0-L1-level0": ("L0", "L1", "pts596", 0),
    "L0-L1-level4": ("L0", "L1", "pts596", 4),
    "flat": ("flat", "flat", "flat50", 3),
    "crop": ("cL0", "cL1", "crop60", 3),
    "crop-level0": ("cL0", "cL1", "crop60", 0),
    "crop-level4": ("cL0", "cL1", "crop60", 4),
    "lattice": ("cL0", "cL1", "lattice", 3),
}


def freeze(want):
    for arr in want:
        if arr is not None:
            arr.setflags(write=False)
    return want


def case(name, small_seq, orc):
    """dict(prev, next, pts, max_level, want=(next, status, err)) of a named case; the checker runs once per session"""
    if name not in _CACHE:
        a, b, p, ml = CASES[name]
        im, ps = images(small_seq), point_sets(small_seq)
        want = freeze(orc.calc_optical_flow_pyr_lk(im[a], im[b], ps[p], max_level=ml))
        _CACHE[name] = dict(prev=im[a], next=im[b], pts=ps[p], max_level=ml, want=want)
    return _CACHE[name]


def random_draw(rng, seed, small_seq):
    """(prev, next, pts, max_level): a crop of 64 .. 200 x 48 .. 160 of L0 -> L1, n of 0 .. 128 points (seed 0: none, seed 1: one)
    uniform in [-25, w + 25] x [-25, h + 25], and a max_level of 0 .. 4"""
    w, h = int(rng.integers(64, 201)), int(rng.integers(48, 161))
    x0, y0 = int(rng.integers(0, 480 - w + 1)), int(rng.integers(0, 160 - h + 1))
    n = 0 if seed == 0 else 1 if seed == 1 else int(rng.integers(0, 129))
    prev = np.ascontiguousarray(small_seq["L"][0][y0:y0 + h, x0:x0 + w])
    nxt = np.ascontiguousarray(small_seq["L"][1][y0:y0 + h, x0:x0 + w])
    pts = np.stack([rng.uniform(-25, w + 25, n), rng.uniform(-25, h + 25, n)], -1).astype(np.float32).reshape(-1, 2)
    return prev, nxt, pts, int(rng.integers(0, 5))


def no_points():
    return np.zeros((0, 2), np.float32), np.zeros(0, np.uint8), np.zeros(0, np.float32)


def random_case(seed, small_seq, orc):
    """random_draw of generator 1000 + seed, tracked at its max_level"""
    key = ("random", seed)
    if key not in _CACHE:
        prev, nxt, pts, ml = random_draw(np.random.default_rng(1000 + seed), seed, small_seq)
        want = orc.calc_optical_flow_pyr_lk(prev, nxt, pts, max_level=ml) if len(pts) else no_points()
        _CACHE[key] = dict(prev=prev, next=nxt, pts=pts, max_level=ml, want=want)
    return _CACHE[key]


def assert_not_vacuous(name, c):
    """the checker's side of a comparison: both statuses, the tracked-but-left-the-image quirk and the zero-err rule occur"""
    nxt, st, err = c["want"]
    assert np.all(err[st == 0] == 0), "err of a status-0 point is exactly 0"
    neg = (st == 1) & ((nxt[:, 0] < 0) | (nxt[:, 1] < 0))
    if c["pts"].shape[0] == 596:
        assert len(st) == 596 and (st == 1).sum() >= 500 and (st == 0).sum() >= 20
        if c["prev"] is not c["next"]:
            assert neg.sum() >= 1
            assert np.all(err[st == 1] > 0), "a moving pair: non-zero err on every tracked point"
        else:
            assert np.all(err == 0)
    elif name == "flat":
        assert (st == 0).all()
    elif name.startswith("crop"):
        assert (st == 1).sum() >= 50 and (st == 0).sum() >= 1
    elif name == "lattice":
        assert (st == 1).sum() >= 50 and (st == 0).sum() >= 50


def delete_unmatch_features(points0, points1, status):
    """feature.cpp:20-37: a tracked point with a negative coordinate gets status 0; points with status 0 are erased from both
    vectors, the status vector keeps its length"""
    status = status.copy()
    keep = []
    for i in range(len(status)):
        if status[i] and (points1[i, 0] < 0 or points1[i, 1] < 0):
            status[i] = 0
        if status[i]:
            keep.append(i)
    keep = np.array(keep, np.int32).reshape(-1)
    return points0[keep], points1[keep], status, keep


def assert_same(got, want, what=""):
    """positions, status and err bit for bit, every point"""
    gn, gs, ge = got
    wn, ws, we = want
    assert np.array_equal(gs, ws), (what, "status", np.flatnonzero(gs != ws)[:8])
    assert np.array_equal(bits(gn), bits(wn)), (what, "positions", np.flatnonzero((bits(gn) != bits(wn)).any(1))[:8])
    if ge is not None:
        assert np.array_equal(bits(ge), bits(we)), (what, "err", np.flatnonzero(bits(ge) != bits(we))[:8])
