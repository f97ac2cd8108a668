"""Rectification maps for vo_params.rectify (include/vo_hip.h, RECTIFICATION): cv::initUndistortRectifyMap without OpenCV.

    map_x, map_y = init_undistort_rectify_map(K, D, R, P, w, h)          # two (h, w) float32 arrays, CV_32FC1 like OpenCV's
    vo = StereoOdometry(P_l, P_r, ..., rectify=((mx_l, my_l), (mx_r, my_r)))

Host only, once per calibration; the per-frame cv::remap is the library's (csrc/rectify.hip).  C++ callers pass OpenCV's own maps.

The algorithm is OpenCV's (calib3d, initUndistortRectifyMap, m1type = CV_32FC1) in numpy float64, every value rounded to float32
once at the end, with + - * / only, in THIS order (tests/test_rectify_abi.py restates it as a scalar loop and compares bit for bit):
    A  = P[:, :3] @ R, each entry (a0 * b0 + a1 * b1) + a2 * b2
    iR = inverse of A by cofactors: entry (i, j) = cofactor(j, i) / det, det = (A00 * c00 + A01 * c01) + A02 * c02,
         each cofactor of the form a * b - c * d
    for the destination pixel (u, v) = (column, row):
        X = (iR00 * u + iR01 * v) + iR02,  Y = (iR10 * u + iR11 * v) + iR12,  W = (iR20 * u + iR21 * v) + iR22
        x = X / W, y = Y / W, x2 = x * x, y2 = y * y, r2 = x2 + y2, xy2 = (2 * x) * y
        kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
        xd = (x * kr + p1 * xy2) + p2 * (r2 + 2 * x2)
        yd = (y * kr + p1 * (r2 + 2 * y2)) + p2 * xy2
        map_x = fx * xd + cx,  map_y = fy * yd + cy                      (fx, fy, cx, cy of K)
(OpenCV walks a row by adding iR's first column to X, Y, W pixel after pixel; the products above are the same quantities without
the accumulated rounding -- the two agree to a few ulp of float64, far below the 1/32-pixel grid the remap rounds to.)
D = (k1, k2, p1, p2[, k3[, k4, k5, k6]]): OpenCV's order, up to 8 coefficients, missing ones 0; R None = identity; P 3x3 or 3x4."""
import numpy as np


def _inv3(A):
    c = [[0.0] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            i0, i1 = [k for k in range(3) if k != i]
            j0, j1 = [k for k in range(3) if k != j]
            m = A[i0][j0] * A[i1][j1] - A[i0][j1] * A[i1][j0]
            c[i][j] = m if (i + j) % 2 == 0 else 0.0 - m
    det = (A[0][0] * c[0][0] + A[0][1] * c[0][1]) + A[0][2] * c[0][2]
    return [[c[j][i] / det for j in range(3)] for i in range(3)]


def init_undistort_rectify_map(K, D, R, P, w, h):
    K = np.asarray(K, np.float64).reshape(3, 3)
    D = np.zeros(0) if D is None else np.asarray(D, np.float64).reshape(-1)
    if D.size > 8:
        raise ValueError("up to 8 distortion coefficients (k1, k2, p1, p2, k3, k4, k5, k6)")
    k1, k2, p1, p2, k3, k4, k5, k6 = [float(v) for v in np.concatenate([D, np.zeros(8 - D.size)])]
    R = np.eye(3) if R is None else np.asarray(R, np.float64).reshape(3, 3)
    P = K if P is None else np.asarray(P, np.float64)
    P = P.reshape(3, -1)[:, :3]
    A = [[(float(P[i, 0]) * float(R[0, j]) + float(P[i, 1]) * float(R[1, j])) + float(P[i, 2]) * float(R[2, j]) for j in range(3)]
         for i in range(3)]
    iR = _inv3(A)
    fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    u = np.arange(w, dtype=np.float64)[None, :]
    v = np.arange(h, dtype=np.float64)[:, None]
    X = (iR[0][0] * u + iR[0][1] * v) + iR[0][2]
    Y = (iR[1][0] * u + iR[1][1] * v) + iR[1][2]
    W = (iR[2][0] * u + iR[2][1] * v) + iR[2][2]
    x, y = X / W, Y / W
    x2, y2 = x * x, y * y
    r2 = x2 + y2
    xy2 = (2.0 * x) * y
    kr = (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2)
    xd = (x * kr + p1 * xy2) + p2 * (r2 + 2.0 * x2)
    yd = (y * kr + p1 * (r2 + 2.0 * y2)) + p2 * xy2
    return (fx * xd + cx).astype(np.float32), (fy * yd + cy).astype(np.float32)


def stereo_maps(left, right, w, h):
    """((map_x_left, map_y_left), (map_x_right, map_y_right)) from two calibration records with K, D, R, P (dicts, e.g. what
    visual_odom_amd.run.read_rectification returns): the `rectify=` argument of StereoOdometry / MultiSequenceOdometry"""
    return tuple(init_undistort_rectify_map(c["K"], c.get("D"), c.get("R"), c.get("P"), w, h) for c in (left, right))
