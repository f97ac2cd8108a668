"""The seeded fuzz of the detector with a response (include/vo_corners_response.h): 60 cases from one seed, a plain list, so that the
SAME cases run on the device (test_gpu_corners_response.py: all of them, none may be skipped) and a few of them through the
coroutine emulator on the CPU (test_corners_response_emulation.py).  A case is a region of one of three 160 x 160 sources with
sizes 32 .. 160, a random response (the default one included), k, mask, min_distance, quality_level and max_corners.  Expected
values are tests/host_check/corners_response_ref.c's; everything is identity."""
import numpy as np

import corners_emu as ce
import corners_mask_cases as cm
import corners_response_cases as cr

SEED = 20240607
N_CASES = 60
SRC = 160
RESPONSES = [(3, 0), (5, 0), (3, 1), (5, 1)]
KS = [0.04, 0.04, 0.0, -0.1, 0.06, 0.25]
DISTANCES = [0.0, 0.5, 1.0, 1.5, 2.5, 5.0, 7.5, 10.5, 17.3]
QUALITIES = [1e-3, 0.01, 0.01, 0.05, 0.3, 1.0]
MAX_CORNERS = [0, 0, 1, 17, 500]
MASKS = [None, None, cm.left_half, cm.checker, lambda w, h: cm.random_half(w, h, 5), lambda w, h: np.zeros((h, w), np.uint8)]


def sources():
    return [ce.noise(SRC, SRC, 51), ce.blobs(SRC, SRC, 52, count=90), ce.squares(SRC, SRC, 53)]


def cases():
    """[dict(img (a view: stride 160), mask or None, block, harris, k, md, q, mc)]"""
    rng = np.random.default_rng(SEED)
    srcs = sources()
    out = []
    for i in range(N_CASES):
        w, h = int(rng.integers(32, SRC + 1)), int(rng.integers(32, SRC + 1))
        x0, y0 = int(rng.integers(0, SRC - w + 1)), int(rng.integers(0, SRC - h + 1))
        block, harris = RESPONSES[i % 4] if i < 8 else RESPONSES[int(rng.integers(0, 4))]   # (every response at least twice)
        gen = MASKS[int(rng.integers(0, len(MASKS)))]
        out.append(dict(img=srcs[int(rng.integers(0, 3))][y0:y0 + h, x0:x0 + w], mask=None if gen is None else gen(w, h), block=block, harris=harris,
                        k=KS[int(rng.integers(0, len(KS)))], md=DISTANCES[int(rng.integers(0, len(DISTANCES)))],
                        q=QUALITIES[int(rng.integers(0, len(QUALITIES)))], mc=MAX_CORNERS[int(rng.integers(0, len(MAX_CORNERS)))]))
    return out


def expected(c):
    """(map, corners, n) of the reference"""
    img = np.ascontiguousarray(c["img"])
    pts, n, _ = cr.ref_detect(img, c["mask"], c["mc"], c["q"], c["md"], c["block"], c["harris"], c["k"])
    return cr.ref_map(img, c["block"], c["harris"], c["k"]), pts, n
