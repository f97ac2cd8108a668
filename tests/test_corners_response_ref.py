"""tests/host_check/corners_response_ref.c -- the restatement of cv::cornerMinEigenVal(B, 3), cv::cornerHarris(B, 3, k) and
cv::goodFeaturesToTrack(..., mask, B, useHarris, k) the device path of include/vo_corners_response.h is held to -- checked against
things that are not itself: corners_ref.c and corners_mask_cases.ref_detect at (3, min-eigen), an independent numpy f64 computation
of the other maps, and the premises the device tests rest on, each shown from the reference alone.  CPU only."""
import numpy as np
import pytest

import corners_emu as ce
import corners_mask_cases as cm
import corners_response_cases as cr

EPS = float(np.finfo(np.float32).eps)
SHAPES = [(3, 3), (5, 4), (17, 13), (65, 17), (131, 67)]


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_at_3_min_eigen_it_is_corners_ref_bit_for_bit(shape):
    w, h = shape
    for name, img in (("noise", ce.noise(w, h, 1)), ("blobs", ce.blobs(w, h, 2)), ("dark", ce.dark_highlights(w, h, 3)), ("periodic", ce.periodic(w, h))):
        for trap, order in ((0, 0), (1, 0), (0, 1)):
            assert np.array_equal(cr.bits(cr.ref_map(img, 3, 0, trap=trap, order=order)), cr.bits(ce.ref_map(img, trap=trap, order=order))), (name, trap, order)
        assert np.array_equal(cr.bits(cr.ref_map(img, 3, 0, stride=w + 7)), cr.bits(ce.ref_map(img))), name
        for mc, q, md in ((0, 0.01, 5.0), (0, 0.05, 0.0), (7, 0.01, 1.0), (0, 0.3, 10.5)):
            want, n, nc = ce.ref_detect(img, mc, q, md)
            got, m, mnc = cr.ref_detect(img, None, mc, q, md)
            assert (m, mnc) == (n, nc) and got.tobytes() == want.tobytes(), (name, mc, q, md)


@pytest.mark.parametrize("shape", [(32, 32), (65, 33), (131, 67)], ids=lambda s: "%dx%d" % s)
def test_under_a_mask_it_is_the_mask_reference(shape):
    w, h = shape
    for name, img, mask, mc, q, md in cm.mask_cases(w, h):
        want, n, nc = cm.ref_detect(img, mask, mc, q, md)
        got, m, mnc = cr.ref_detect(img, mask, mc, q, md)
        assert (m, mnc) == (n, nc) and got.tobytes() == want.tobytes(), name


def numpy_map(img, block, harris, k):
    """the response in f64 from the definitions: Sobel 3 x 3 / (255 * 4 * B) on the REFLECT_101 image, products, B x B box sum of the
    REFLECT_101 product images, then the smaller eigenvalue of [[a / 2, b], [b, c / 2]] or a c - b^2 - k (a + c)^2"""
    r = block // 2
    p = np.pad(img.astype(np.float64), 1, mode="reflect")
    s = 1.0 / (255.0 * 4.0 * block)
    dx = ((p[:-2, 2:] - p[:-2, :-2]) + 2 * (p[1:-1, 2:] - p[1:-1, :-2]) + (p[2:, 2:] - p[2:, :-2])) * s
    dy = ((p[2:, :-2] - p[:-2, :-2]) + 2 * (p[2:, 1:-1] - p[:-2, 1:-1]) + (p[2:, 2:] - p[:-2, 2:])) * s

    def box(c):
        q = np.pad(c, r, mode="reflect")
        h, w = c.shape
        return sum(q[j:j + h, i:i + w] for j in range(block) for i in range(block))
    a, b, c = box(dx * dx), box(dx * dy), box(dy * dy)
    if harris:
        return a * c - b * b - k * (a + c) ** 2
    a, c = a * 0.5, c * 0.5
    return (a + c) - np.sqrt((a - c) ** 2 + b * b)


IMAGES = [("noise", ce.noise(131, 67, 1)), ("blobs", ce.blobs(131, 67, 2)), ("squares", ce.squares(65, 17, 3)), ("tiny", ce.noise(5, 5, 4)),
          ("noise_small", ce.noise(17, 13, 2))]


@pytest.mark.parametrize("block,harris", cr.RESPONSES)
@pytest.mark.parametrize("name,img", IMAGES, ids=[n for n, _ in IMAGES])
def test_map_agrees_with_an_independent_f64_computation(name, img, block, harris):
    """test_corners_ref.py's bound, 4 f32 ulp of the map's largest value (a Harris map has values of both signs: the largest
    magnitude).  The f32 chain rounds dx, dy, the products, the cast of the f64 sum and the operations of the response, each a
    relative 2^-24 of a quantity bounded by the trace (its square for Harris), whose largest value is within a small factor of the
    map's on an image with corners; measured figures are printed"""
    ref = cr.ref_map(img, block, harris, cr.K)
    want = numpy_map(img, block, harris, cr.K)
    err = np.abs(ref.astype(np.float64) - want).max()
    ulp = EPS * max(float(np.abs(want).max()), 1e-30)
    print(name, block, harris, "max |ref - f64| = %.3g = %.2f ulp of the map's largest magnitude" % (err, err / ulp))
    assert err <= 4 * ulp


def differing(a, b):
    return int((cr.bits(a) != cr.bits(b)).sum())


def test_premise_a_the_trap_matters_at_block_5():
    """cov of the reflected SOURCE is not the reflected cov: on a one-sided border dx dy changes sign, two samples deep at B = 5"""
    for harris in (0, 1):
        img = cr.one_sided(65, 33, 6)
        a, b = cr.ref_map(img, 5, harris), cr.ref_map(img, 5, harris, trap=1)
        d = cr.bits(a) != cr.bits(b)
        print("harris", harris, "pixels that differ under the trap:", int(d.sum()))
        assert d.any() and not d[4:-4, 4:-4].any(), "the border band, and nothing else"
        assert cr.ref_detect(img, None, 0, 0.01, 1.0, 5, harris)[0].tobytes() != cr.ref_detect(img, None, 0, 0.01, 1.0, 5, harris, trap=1)[0].tobytes()


def test_premise_b_the_running_column_sum_is_not_order_free_at_block_5():
    differ = 0
    for seed in range(4):
        img = ce.dark_highlights(131, 67, seed)
        n = differing(cr.ref_map(img, 5, 0), cr.ref_map(img, 5, 0, order=1))
        print(seed, "pixels that differ:", n)
        differ += n > 0
    assert differ == 4


def test_premise_c_the_vector_form_of_harris_differs_from_the_scalar_text():
    """form 1, the f32 loop of a vectorised build, against form 0, the scalar text that is the specification: the share of noise
    pixels whose last bits differ (DESIGN 6 records the figures printed here)"""
    for block in (3, 5):
        img = ce.noise(48, 40, 9)
        n = differing(cr.ref_map(img, block, 1), cr.ref_map(img, block, 1, form=1))
        print("block", block, "pixels that differ between the forms: %d of %d = %.1f %%" % (n, img.size, 100.0 * n / img.size))
        assert n > 0
        assert differing(cr.ref_map(img, block, 0), cr.ref_map(img, block, 0, form=1)) == 0, "the switch touches Harris alone"


def test_premises_d_e_block_size_and_response_change_the_corner_list():
    img = ce.noise(131, 67, 12)
    lists = {(b, hr): cr.ref_detect(img, None, 0, 0.01, 5.0, b, hr)[0].tobytes() for b in (3, 5) for hr in (0, 1)}
    assert lists[(3, 0)] != lists[(5, 0)] and lists[(3, 1)] != lists[(5, 1)]          # d
    assert lists[(3, 0)] != lists[(3, 1)] and lists[(5, 0)] != lists[(5, 1)]          # e
    assert cr.ref_detect(img, None, 0, 0.01, 5.0, 3, 1, 0.04)[0].tobytes() != cr.ref_detect(img, None, 0, 0.01, 5.0, 3, 1, 0.25)[0].tobytes()


RAMP_CANDIDATES = {3: 840, 5: 840}   # the reference's own counts on the 32 x 32 ramp at quality_level 3


def test_the_negative_maximum():
    """a Harris map that is negative everywhere: (float)(max * q) lies ABOVE every value for q < 1 -- threshold(TOZERO) zeroes the
    map and there is no corner -- and below them for q > 1, where the negative plateau survives as it is and its ties are all
    candidates.  Selection is literal about sign"""
    img = cr.ramp(32, 32)
    for block in (3, 5):
        m = cr.ref_map(img, block, 1)
        assert (m < 0).all(), block
        assert cr.ref_detect(img, None, 0, 0.01, 0.0, block, 1)[1:] == (0, 0)
        pts, n, nc = cr.ref_detect(img, None, 0, 3.0, 0.0, block, 1)
        print("block", block, "candidates at quality 3:", nc)
        assert n == nc == RAMP_CANDIDATES[block]
        best = m[1:-1, 1:-1].max()
        assert m[int(pts[0, 1]), int(pts[0, 0])] == best, "the list starts at the largest (least negative) value"
        # with minDistance the same candidates thin out, still in descending order of a negative quality
        p5, n5, nc5 = cr.ref_detect(img, None, 0, 3.0, 5.0, block, 1)
        q5 = m[p5[:, 1].astype(int), p5[:, 0].astype(int)]
        assert nc5 == nc and 0 < n5 < n and (np.diff(q5) <= 0).all()
