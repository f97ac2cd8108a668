"""tests/host_check/corners_ref.c -- the restatement of cv::cornerMinEigenVal(3, 3) / cv::goodFeaturesToTrack the device path of
include/vo_corners.h is held to -- checked against things that are not itself: an independent numpy f64 computation of the
quality map, and brute-force properties of the detector's output (local maxima above the threshold, order, the cell rule of the
suppression, maximality).  CPU only."""
import ctypes as C

import numpy as np
import pytest

import corners_emu as ce

EPS = float(np.finfo(np.float32).eps)


def numpy_map(img):
    """the quality map in f64 from the definitions: Sobel 3 x 3 / (255 * 12) on the REFLECT_101 image, products, 3 x 3 box sum of the
    REFLECT_101 product images, smaller eigenvalue of [[a, b], [b, c]] with a = sxx / 2, b = sxy, c = syy / 2"""
    p = np.pad(img.astype(np.float64), 1, mode="reflect")
    s = 1.0 / (255.0 * 12.0)
    dx = ((p[:-2, 2:] - p[:-2, :-2]) + 2 * (p[1:-1, 2:] - p[1:-1, :-2]) + (p[2:, 2:] - p[2:, :-2])) * s
    dy = ((p[2:, :-2] - p[:-2, :-2]) + 2 * (p[2:, 1:-1] - p[:-2, 1:-1]) + (p[2:, 2:] - p[:-2, 2:])) * s

    def box(c):
        q = np.pad(c, 1, mode="reflect")
        h, w = c.shape
        return sum(q[j:j + h, i:i + w] for j in range(3) for i in range(3))
    a, b, c = box(dx * dx) * 0.5, box(dx * dy), box(dy * dy) * 0.5
    return (a + c) - np.sqrt((a - c) ** 2 + b * b), a + c


IMAGES = [("noise", ce.noise(131, 67, 1)), ("blobs", ce.blobs(131, 67, 2)), ("squares", ce.squares(65, 17, 3)), ("periodic", ce.periodic(64, 16)),
          ("border_max", ce.border_max(65, 17)), ("tiny", ce.noise(5, 4, 4)), ("noise_small", ce.noise(17, 13, 2))]


@pytest.mark.parametrize("name,img", IMAGES, ids=[n for n, _ in IMAGES])
def test_map_agrees_with_an_independent_f64_computation(name, img):
    """a few f32 ulp of the map maximum: the f32 chain rounds dx, dy (3 roundings each), the products, the cast of the f64 sum and
    the four operations of the eigenvalue -- each a relative 2^-24 of a quantity bounded by the trace a + c, whose largest value is
    within a small factor of the map maximum on an image with corners; measured figures are printed"""
    ref = ce.ref_map(img)
    want, trace = numpy_map(img)
    err = np.abs(ref.astype(np.float64) - want).max()
    ulp = EPS * max(float(want.max()), 1e-30)
    print(name, "max |ref - f64| = %.3g = %.2f ulp of the map maximum; trace max / map max = %.2f" % (err, err / ulp, trace.max() / max(want.max(), 1e-30)))
    assert err <= 4 * ulp


def test_the_running_column_sum_is_not_order_free():
    """`order` 1 of the ref is a plain three-term column sum.  It equals upstream's running sum (order 0, the specification) only
    while the f64 operations are exact; on a dark frame with highlights above a flat area they are not, and the residual stays in
    the running sum for the rest of the column"""
    differ = 0
    for seed in range(4):
        img = ce.dark_highlights(131, 67, seed)
        a, b = ce.ref_map(img), ce.ref_map(img, order=1)
        differ += int((a.view(np.uint32) != b.view(np.uint32)).any())
        print(seed, "pixels that differ:", int((a.view(np.uint32) != b.view(np.uint32)).sum()), "max |diff| %.3g" % np.abs(a.astype(np.float64) - b).max())
    assert differ == 4


def conflicts(p, q, md):
    """upstream's rule: q is looked at from p only inside the 3 x 3 cells around p's cell (cell = cvRound(md), half to even), and
    rejects when the f32 squared distance is below md^2"""
    cell = int(np.rint(md))
    if abs(int(p[0]) // cell - int(q[0]) // cell) > 1 or abs(int(p[1]) // cell - int(q[1]) // cell) > 1:
        return False
    d = np.float32(p[0] - q[0]) ** 2 + np.float32(p[1] - q[1]) ** 2
    return float(d) < md * md


def candidates_brute(img, q):
    """(x, y, value) of every interior 3 x 3 maximum of the thresholded map, best first, ties by the higher address"""
    m = ce.ref_map(img)
    thr = np.float32(float(m.max()) * q)
    t = np.where(m > thr, m, np.float32(0))
    h, w = m.shape
    out = []
    for y in range(1, h - 1):
        for x in range(1, w - 1):
            if t[y, x] != 0 and t[y, x] == t[y - 1:y + 2, x - 1:x + 2].max():
                out.append((float(t[y, x]), y * w + x))
    out.sort(reverse=True)
    return [(i % w, i // w, v) for v, i in out], t


@pytest.mark.parametrize("name,img", IMAGES[:5], ids=[n for n, _ in IMAGES[:5]])
@pytest.mark.parametrize("md", [0.0, 1.0, 5.0, 10.5, 32.0])
def test_detector_output_has_the_properties_of_the_serial_loop(name, img, md):
    q = 0.02
    pts, n, nc = ce.ref_detect(img, 0, q, md)
    cand, t = candidates_brute(img, q)
    assert nc == len(cand) and n == len(pts)
    h, w = img.shape
    val = [t[int(y), int(x)] for x, y in pts]
    cset = {(x, y) for x, y, _ in cand}
    for (x, y), v in zip(pts, val):                                   # interior 3 x 3 maxima above the threshold
        assert (int(x), int(y)) in cset and v > 0
    assert all(val[i] >= val[i + 1] for i in range(n - 1))            # qualities are non-increasing
    addr = [int(y) * w + int(x) for x, y in pts]
    assert all(addr[i] > addr[i + 1] for i in range(n - 1) if val[i] == val[i + 1])   # equal qualities: descending address
    if md < 1:
        assert [(int(x), int(y)) for x, y in pts] == [(x, y) for x, y, _ in cand]
        return
    for i in range(n):                                                # no two corners in conflict
        for j in range(i):
            assert not conflicts(pts[i], pts[j], md), (pts[i], pts[j])
    got = {(int(x), int(y)) for x, y in pts}
    rank = {(x, y): k for k, (x, y, _) in enumerate(cand)}
    for x, y, _ in cand:                                              # maximal: a dropped candidate conflicts with a better accepted one
        if (x, y) not in got:
            assert any(rank[(int(px), int(py))] < rank[(x, y)] and conflicts((x, y), (px, py), md) for px, py in pts), (x, y)


def test_hand_built_cases():
    flat = np.full((13, 17), 77, np.uint8)
    assert ce.ref_detect(flat, 0, 0.01, 5)[1:] == (0, 0) and not ce.ref_map(flat).any()
    for shape in ((2, 17), (13, 2), (1, 1), (2, 2)):
        assert ce.ref_detect(ce.noise(shape[1], shape[0], 1), 0, 0.01, 5)[1] == 0
    img = ce.noise(65, 17, 3)
    assert ce.ref_detect(img, 0, 1.0, 5)[1] == 0          # nothing is above the maximum itself
    full = ce.ref_detect(img, 0, 0.01, 5)[0]
    assert len(full) > 7 and np.array_equal(ce.ref_detect(img, 7, 0.01, 5)[0], full[:7])   # max_corners: a prefix
    assert np.array_equal(ce.ref_detect(img, 0, 0.01, 5, cap=3)[0], full[:3]) and ce.ref_detect(img, 0, 0.01, 5, cap=3)[1] == len(full)
    lib = ce.load_ref()
    for bad in ((0.0, 5.0, 0), (-1.0, 5.0, 0), (0.01, -1.0, 0), (0.01, 5.0, -1), (float("nan"), 5.0, 0)):
        assert lib.cr_detect(img.ctypes.data, 65, 17, 65, bad[2], bad[0], bad[1], None, 0, None, 0) == -1


def test_cell_size_rounds_half_to_even():
    """min_distance 10.5 and 11.5 give cells 10 and 12 (cvRound: half to even).  The cell size is not visible in the output: two
    pixels closer than min_distance differ by at most ceil(min_distance) - 1 <= cvRound(min_distance) in each coordinate, so their
    cells are always neighbours -- which the brute-force check confirms at both distances with ANY pair closer than min_distance
    counted as a conflict, cells ignored"""
    lib = ce.load_ref()
    assert [lib.cr_cell(C.c_double(md)) for md in (10.5, 11.5, 1.0, 1.5, 2.5, 32.0)] == [10, 12, 1, 2, 2, 32]
    img = ce.noise(131, 67, 6)
    for md in (10.5, 11.5):
        pts, n, _ = ce.ref_detect(img, 0, 0.02, md)
        cand, _ = candidates_brute(img, 0.02)
        kept = []
        for x, y, _ in cand:   # the greedy loop without cells
            if all((x - px) ** 2 + (y - py) ** 2 >= md * md for px, py in kept):
                kept.append((x, y))
        assert [(int(x), int(y)) for x, y in pts] == kept
