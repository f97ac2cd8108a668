"""The Shi-Tomasi detector where corn_select_kernel and corn_map_kernel change behaviour: the case table test_corners_scale_emulation.py
(the coroutine emulator) and test_gpu_corners_scale.py (the device) share.  corn_select_kernel runs 1024 threads, so a list of more
than 1024 candidates makes every strided loop take several trips, more than 2048 make the bitonic sort's inner loop take several,
and a list that is no power of two is padded for the sort; corn_map_kernel owns 254 columns per workgroup, with one halo column each
side through LDS, so widths 254, 255, 256, 508 and 509 sit on both sides of a seam.

Every case states its PREMISE -- what makes it the case it is called: its candidate count, the corners it keeps -- and premise()
asserts it from the reference alone (corners_emu.ref_detect, corners_mask_cases.ref_detect) before anything is compared.  The
reference's answer of a case is computed once per session and shared."""
import collections
import functools

import numpy as np

import corners_emu as ce
import corners_mask_cases as cm

CAPACITY = 16384   # the corner-list capacity of a context up to 512 x 512 pixels and 4096 points (include/vo_hip.h)

# premise: candidates, corners (None: whatever the reference gives); deep: the suppression takes >= 100 rounds (the emulator reports
# them); over: one candidate more than CAPACITY, the run is refused.  The quality map of every distinct image is compared too
Case = collections.namedtuple("Case", "name img max_corners quality min_distance candidates corners deep over")


def _case(name, img, mc=0, q=0.01, md=5.0, candidates=None, corners=None, deep=False, over=False):
    img.setflags(write=False)
    return Case(name, img, mc, q, md, candidates, corners, deep, over)


def tiles(w, h, cols=None):
    """a 3 x 3 tile repeated over the first `cols` columns (default: all), flat beyond: the 3 x 3 box sums of a pattern of period 3
    are the same at every pixel, so the quality map is one exact plateau there and every interior pixel of it is a candidate"""
    tile = np.random.default_rng(1).integers(0, 256, (3, 3), dtype=np.uint8)
    img = np.full((h, w), 128, np.uint8)
    cols = w if cols is None else cols
    img[:, :cols] = np.tile(tile, (h // 3 + 1, w // 3 + 1))[:h, :cols]
    return img


def one_over():
    """the full list and one isolated dot in the flat part: 16 385 candidates"""
    img = tiles(256, 132, 132)
    img[60, 200] = 255
    return img


SEAM_WIDTHS = [254, 255, 256, 300, 508, 509]
SEAM_HEIGHTS = [33, 40]
DISTANCES = [0.5, 0.99, 1.0, 1.2, 1.41, 1.5, 2.5, 3.5, 100.0, 256.0]
PLATEAU = (131, 67, 60)   # tiles(): 3 528 candidates, no power of two (the sort runs over 4 096 keys, two trips)


def _build():
    full, short, over, plateau = tiles(256, 132, 132), tiles(256, 132, 131), one_over(), tiles(*PLATEAU)
    groups = collections.OrderedDict()
    groups["full-list"] = [_case("full-list-md0", full, md=0.0, candidates=16384, corners=16384),
                           _case("full-list-md1.2", full, md=1.2, candidates=16384, corners=8192, deep=True),
                           _case("full-list-md5", full, md=5.0, candidates=16384, corners=676, deep=True)]
    groups["one-short"] = [_case("one-short-md0", short, md=0.0, candidates=16383, corners=16383),
                           _case("one-short-md1.2", short, md=1.2, candidates=16383, corners=8193, deep=True),
                           _case("one-short-md5", short, md=5.0, candidates=16383, corners=676, deep=True)]
    groups["one-over"] = [_case("one-over-md0", over, md=0.0, candidates=16385, over=True),
                          _case("one-over-md1.2", over, md=1.2, candidates=16385, over=True)]
    groups["plateau"] = [_case("plateau-131x67-md1.2", plateau, md=1.2, candidates=3528, corners=1764, deep=True),
                         _case("plateau-131x67-md5", plateau, md=5.0, candidates=3528, corners=156)]
    seams = []
    for w in SEAM_WIDTHS:
        for h in SEAM_HEIGHTS:
            for cname, img in (("noise", ce.noise(w, h, 1)), ("dark_highlights", ce.dark_highlights(w, h, 5)), ("periodic", ce.periodic(w, h, 4))):
                seams.append(_case("seams-%s-%dx%d" % (cname, w, h), img, md=3.0))
    seams.append(_case("seams-periodic-512x64", ce.periodic(512, 64, 4), md=3.0, candidates=3953))
    groups["seams"] = seams
    groups["distances"] = [_case("distances-%s-md%g" % (cname, md), img, md=md)
                           for cname, img in (("noise", ce.noise(131, 67, 1)), ("tiles", plateau)) for md in DISTANCES]
    # max_corners inside a long list: 1 (the first trip's first thread), 1025 (one past the first trip), n - 1; without suppression
    # (the list's first max_corners) and with it (the scan's cut)
    groups["limit-in-a-long-list"] = ([_case("limit-md0-max%d" % mc, plateau, mc=mc, md=0.0, candidates=3528, corners=mc) for mc in (1, 1025, 3527)]
                                      + [_case("limit-md1.2-max%d" % mc, plateau, mc=mc, md=1.2, candidates=3528, corners=mc) for mc in (1, 1025, 1763)])
    return groups


GROUPS = _build()
SCALE_CASES = [c for g in GROUPS.values() for c in g]
assert len({c.name for c in SCALE_CASES}) == len(SCALE_CASES)


def left_columns(w, h, cols=30):
    m = np.zeros((h, w), np.uint8)
    m[:, :cols] = 255
    return m


# the same plateau under a mask: (name, image, mask, max_corners, quality, min_distance), against corners_mask_cases.ref_detect.
# left_half (value 1) ends in the flat part beyond the pattern's 60 columns: every candidate stays, through the masked kernels;
# checker and left_columns cut through the plateau
MASK_CASES = [("plateau-%s-md%g" % (mname, md), tiles(*PLATEAU), gen(PLATEAU[0], PLATEAU[1]), 0, 0.01, md)
              for mname, gen in (("checker", cm.checker), ("left_half", cm.left_half), ("left_columns", left_columns)) for md in (1.2, 5.0)]


@functools.lru_cache(maxsize=None)
def _ref(name):
    c = next(c for c in SCALE_CASES if c.name == name)
    return ce.ref_detect(c.img, c.max_corners, c.quality, c.min_distance)


def premise(c):
    """the reference's (corners, n, candidates) of the case, after asserting what the case claims about itself"""
    pts, n, ncand = _ref(c.name)
    assert c.candidates is None or ncand == c.candidates, (c.name, ncand)
    assert c.corners is None or n == c.corners, (c.name, n)
    assert c.over == (ncand > CAPACITY) and (not c.over or ncand == CAPACITY + 1), (c.name, ncand)
    if c.name.startswith("limit-"):
        assert ce.ref_detect(c.img, 0, c.quality, c.min_distance)[1] > c.max_corners > 0, c.name   # the limit binds
    if c.name.startswith("seams-"):
        assert n > 0 and c.img.shape[1] >= 254, c.name                                               # a workgroup's last column, or beyond
    return pts, n, ncand


_MAPS = {}


def ref_map(c):
    """the reference's quality map of the case's image (cases that share an image share it)"""
    if id(c.img) not in _MAPS:
        _MAPS[id(c.img)] = ce.ref_map(c.img)
    return _MAPS[id(c.img)]


@functools.lru_cache(maxsize=None)
def mask_ref(name):
    """corners_mask_cases.ref_detect of a MASK_CASES entry; premise: the mask takes candidates away and leaves more than 1024 -- or,
    left_half, leaves them all"""
    _, img, mask, mc, q, md = next(m for m in MASK_CASES if m[0] == name)
    pts, n, ncand = cm.ref_detect(img, mask, mc, q, md)
    plain = ce.ref_detect(img, mc, q, md)
    if "left_half" in name:
        assert ncand == 3528 and n == plain[1] and np.array_equal(pts, plain[0]) and mask.max() == 1, (name, n, ncand)
    else:
        assert 1024 < ncand < 3528 and 0 < n < plain[1], (name, n, ncand)
    return pts, n, ncand
