"""Shared by tests/test_rectify_emulation.py and tests/test_gpu_rectify.py: the numpy restatement of the rectification formula
of include/vo_hip.h (RECTIFICATION) -- the comparator -- and the maps and images of the cases.  Not a test file."""
import numpy as np

WIDTHS, HEIGHTS = (32, 33, 39, 64, 519), (32, 37)
MAP_KINDS = ("identity", "all_ab", "ties", "barrel", "edges")


def remap_ref(src, map_x, map_y):
    """cv::remap(src, dst, map_x, map_y, INTER_LINEAR, BORDER_CONSTANT, 0), CV_8UC1 / CV_32FC1, in OpenCV's fixed-point form"""
    h, w = src.shape

    def fix(m):
        with np.errstate(invalid="ignore", over="ignore"):
            v = np.asarray(m, np.float32) * np.float32(32)       # exact in f32 (or infinite)
        ok = np.isfinite(v) & (np.abs(v) < 2.0 ** 40)
        s = np.rint(np.where(ok, v, 0)).astype(np.int64)         # half to even
        i = s >> 5
        return np.where(ok, i, -40000), s & 31                   # (a non-finite entry: outside like one that leaves int16)

    ix, a = fix(map_x)
    iy, b = fix(map_y)
    gone = (ix < -32768) | (ix > 32767) | (iy < -32768) | (iy > 32767)
    big = np.zeros((h + 2, w + 2), np.int64)                     # p(j, i) with one pixel of zeros around: taps at -1 .. w, -1 .. h
    big[1:-1, 1:-1] = src
    inside = ~gone & (ix >= -1) & (ix < w) & (iy >= -1) & (iy < h)   # (every other entry has all four taps outside)
    jx, jy = np.where(inside, ix, -1) + 1, np.where(inside, iy, -1) + 1
    p00, p01, p10, p11 = big[jy, jx], big[jy, jx + 1], big[jy + 1, jx], big[jy + 1, jx + 1]
    out = ((32 - a) * (32 - b) * p00 + a * (32 - b) * p01 + (32 - a) * b * p10 + a * b * p11 + 512) >> 10
    return np.where(inside, out, 0).astype(np.uint8)


def make_image(rng, w, h):
    """random pixels with runs of 0 and of 255"""
    img = rng.integers(0, 256, (h, w), dtype=np.uint8)
    img[h // 3, : w // 2] = 0
    img[h // 2, w // 3:] = 255
    img[:, w // 2] = 255
    img[:, w // 2 + 1] = 0
    return img


def barrel_calibration(w, h, k1=-0.3, degrees=1.0, shift=0.25):
    """(K, D, R, P): focal 1.5 w, a destination whose principal point lies `shift` of the image further right and down (its
    top-left corner looks past the source's edge), a small rotation about a tilted axis"""
    K = np.array([[1.5 * w, 0, (w - 1) / 2.0], [0, 1.5 * w, (h - 1) / 2.0], [0, 0, 1]])
    P = K.copy()
    P[0, 2] += shift * w
    P[1, 2] += shift * h
    t = np.deg2rad(degrees)
    ax = np.array([0.5, -0.3, 0.81])
    ax /= np.linalg.norm(ax)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(t) * Kx + (1 - np.cos(t)) * (Kx @ Kx)
    return K, np.array([k1]), R, P


def edge_values(n):
    """the entries of case (e) for an axis of length n"""
    return np.array([-1, -0.5, -1 / 32, n - 1, n - 1 + 1 / 32, n, 1e6, -1e6, np.nan, np.inf, -np.inf], np.float32)


def make_maps(kind, w, h, side=0):
    """(map_x, map_y) float32 (h, w) of one case; side 1 is a DIFFERENT map of the same kind (a swapped side must show)"""
    from visual_odom_amd import rectify
    x = np.tile(np.arange(w, dtype=np.float32), (h, 1))
    y = np.tile(np.arange(h, dtype=np.float32)[:, None], (1, w))
    xi, yi = x.astype(np.int64), y.astype(np.int64)
    if kind == "identity":
        mx, my = x.copy(), y.copy()
        if side:   # (the right side of the identity case: one pixel to the left)
            mx = mx + np.float32(1)
    elif kind == "all_ab":     # every (a, b) pair of the 32 x 32 weights
        mx = x + ((xi + 5 * side) % 32).astype(np.float32) / np.float32(32)
        my = y + ((yi + 3 * side) % 32).astype(np.float32) / np.float32(32)
    elif kind == "ties":       # x * 32 + 0.5 and + 1.5: half to even gives 0 and 2
        mx = x + np.where((xi + yi + side) % 2 == 0, np.float32(1 / 64), np.float32(3 / 64)).astype(np.float32)
        my = y + np.where((xi + side) % 2 == 0, np.float32(3 / 64), np.float32(1 / 64)).astype(np.float32)
    elif kind == "barrel":
        K, D, R, P = barrel_calibration(w, h, degrees=-1.5 if side else 1.0)
        mx, my = rectify.init_undistort_rectify_map(K, D, R, P, w, h)
        assert mx[0, 0] < -1 or my[0, 0] < -1, "the corners of the barrel case leave the image"
    elif kind == "edges":
        mx, my = x + np.float32(0.25 * side), y.copy()
        ex, ey = edge_values(w), edge_values(h)
        for r, row in enumerate((1, h - 2)):          # in x, at the left end of one row and the right end of another
            c0 = 2 if r == 0 else w - 2 - len(ex)
            mx[row, c0:c0 + len(ex)] = ex
        for r, col in enumerate((3, w - 4)):          # in y, down one column and up another
            r0 = 2 if r == 0 else h - 2 - len(ey)
            my[r0:r0 + len(ey), col] = ey
        mx[h // 2, w // 2], my[h // 2, w // 2] = np.nan, np.nan
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(mx, np.float32), np.ascontiguousarray(my, np.float32)


def mild_maps(P_l, w, h):
    """((mx_l, my_l), (mx_r, my_r)) of a mild calibration for the tracking calls: K = the projection's, k1 = -0.05 / -0.045, a
    sub-degree rotation per side (different ones), P = K -- raw frames that still track after rectification"""
    from visual_odom_amd import rectify
    K = np.asarray(P_l, np.float64).reshape(3, 4)[:, :3]
    out = []
    for k1, degrees in ((-0.05, 0.3), (-0.045, -0.25)):
        _, _, R, _ = barrel_calibration(w, h, degrees=degrees)
        out.append(rectify.init_undistort_rectify_map(K, [k1], R, K, w, h))
    return tuple(out)
