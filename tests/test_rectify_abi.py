"""Rectification at ingest (vo_params.rectify) at the interface, without a device: the fields are appended to vo_params behind
input_format (whose offset stays), the ctypes mirror has the C struct's size and offsets, the defaults are off, no entry point
was added, visual_odom_amd.rectify.init_undistort_rectify_map is OpenCV's algorithm (against an independent scalar f64 loop, bit
for bit in f32) and the command line reads ORB-SLAM's stereo calibration layout."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

from visual_odom_amd import _lib, rectify, run

NEW_FIELDS = ("rectify", "rect_w", "rect_h", "rect_map_stride", "rect_map_x_left", "rect_map_y_left", "rect_map_x_right", "rect_map_y_right")
INPUT_FORMAT_OFFSET = 72   # what it was before the fields were appended: 2 int, 2 double, 3 int + 1 float, 1 double, 1 int (+ 4 padding), 2 double
N_EXPORTS = 52            # (51 when rectification came; vo_batch_get_level_planes since)


def test_struct_size_and_offsets_against_a_compiled_probe(tmp_path):
    src = tmp_path / "probe.c"
    names = ("input_format",) + NEW_FIELDS
    src.write_text('#include <stdio.h>\n#include "vo_hip.h"\nint main(void) { printf("%zu", sizeof(vo_params));\n'
                   + "".join('printf(" %%zu", offsetof(vo_params, %s));\n' % n for n in names) + 'printf("\\n"); return 0; }\n')
    exe = str(tmp_path / "probe")
    subprocess.check_call(["gcc", "-include", "stddef.h", "-I" + os.path.join(ROOT, "include"), "-o", exe, str(src)])
    vals = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    assert C.sizeof(_lib.VoParams) == vals[0]
    for n, off in zip(names, vals[1:]):
        assert getattr(_lib.VoParams, n).offset == off, n
    assert vals[1] == INPUT_FORMAT_OFFSET, "input_format stays where it was"
    assert vals[2] == INPUT_FORMAT_OFFSET + 4, "the new fields follow input_format"
    assert vals[0] == vals[-1] + C.sizeof(C.c_void_p), "... and nothing follows them"


def test_header_and_ctypes_layout_declare_the_same_fields():
    """every declarator of the header's struct, comma lists and pointers included, in order, against the ctypes LAYOUT class
    (whose _fields_ is the whole struct; VoParams._fields_ lists the scalars up to input_format only)"""
    import re
    text = open(os.path.join(ROOT, "include", "vo_hip.h")).read()
    body = re.search(r"typedef struct vo_params \{(.*?)\} vo_params;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    ctype = {"int": C.c_int, "float": C.c_float, "double": C.c_double}
    decls = []
    for stmt in body.split(";"):
        stmt = " ".join(stmt.split())
        if not stmt:
            continue
        m = re.match(r"(const )?(int|float|double) (.+)$", stmt)
        assert m, stmt
        for d in m.group(3).split(","):
            d = d.strip()
            ptr = d.startswith("*")
            assert bool(m.group(1)) == ptr, stmt   # (the only pointers are `const float *`)
            decls.append((d.lstrip("* "), C.POINTER(ctype[m.group(2)]) if ptr else ctype[m.group(2)]))
    assert decls == list(_lib._VoParamsLayout._fields_)
    assert [n for n, _ in decls][13:] == list(NEW_FIELDS) and decls[12][0] == "input_format"
    assert _lib.VoParams._fields_ == _lib._VoParamsLayout._fields_[:13] and C.sizeof(_lib.VoParams) == C.sizeof(_lib._VoParamsLayout)


def test_defaults_are_off():
    lib = _lib.load()
    p = _lib.VoParams()
    C.memset(C.byref(p), 0x5A, C.sizeof(p))
    lib.vo_default_params(C.byref(p))
    assert (p.rectify, p.rect_w, p.rect_h, p.rect_map_stride) == (0, 0, 0, 0)
    assert not any(bool(getattr(p, n)) for n in _lib.VoParams.RECT_MAPS)
    assert p.input_format == _lib.FMT_GRAY8 and p.lk_max_level == 3


def test_no_entry_point_was_added():
    assert len(_lib.EXPORTS) == N_EXPORTS
    assert not any("rect" in s or "remap" in s for s in _lib.EXPORTS)


def test_params_helper_points_at_float32_copies_and_switches_off():
    h, w = 34, 40
    maps = ((np.zeros((h, w)), np.ones((h, w))), (np.full((h, w), 2.0), np.full((h, w), 3.0)))   # f64 in: converted once
    p = _lib.VoParams()
    keep = p.set_rectify_maps(maps)
    assert (p.rectify, p.rect_w, p.rect_h, p.rect_map_stride) == (1, w, h, 4 * w)
    assert [a.dtype for a in keep] == [np.float32] * 4 and [float(a[0, 0]) for a in keep] == [0, 1, 2, 3]
    for n, a in zip(_lib.VoParams.RECT_MAPS, keep):
        assert C.cast(getattr(p, n), C.c_void_p).value == a.ctypes.data
    assert p.set_rectify_maps(None) == () and p.rectify == 0 and not bool(p.rect_map_x_left)
    with pytest.raises(ValueError):
        p.set_rectify_maps(((np.zeros((h, w)), np.zeros((h, w))), (np.zeros((h, w)), np.zeros((h, w + 1)))))


def _scalar_maps(K, D, R, P, w, h):
    """OpenCV's initUndistortRectifyMap, one pixel at a time in python floats (IEEE f64), in the operation order
    visual_odom_amd/rectify.py documents; independent of numpy's array code"""
    k = list(D) + [0.0] * (8 - len(D))
    k1, k2, p1, p2, k3, k4, k5, k6 = k
    A = [[(P[i][0] * R[0][j] + P[i][1] * R[1][j]) + P[i][2] * R[2][j] for j in range(3)] for i in range(3)]

    def cof(i, j):
        r = [q for q in range(3) if q != i]
        c = [q for q in range(3) if q != j]
        m = A[r[0]][c[0]] * A[r[1]][c[1]] - A[r[0]][c[1]] * A[r[1]][c[0]]
        return m if (i + j) % 2 == 0 else 0.0 - m
    det = (A[0][0] * cof(0, 0) + A[0][1] * cof(0, 1)) + A[0][2] * cof(0, 2)
    iR = [[cof(j, i) / det for j in range(3)] for i in range(3)]
    fx, fy, cx, cy = K[0][0], K[1][1], K[0][2], K[1][2]
    mx, my = np.zeros((h, w), np.float32), np.zeros((h, w), np.float32)
    for v in range(h):
        for u in range(w):
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
            mx[v, u], my[v, u] = fx * xd + cx, fy * yd + cy
    return mx, my


def _rodrigues(rx, ry, rz):
    r = np.array([rx, ry, rz])
    t = np.linalg.norm(r)
    a = r / t
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * Kx + (1 - np.cos(t)) * (Kx @ Kx)


@pytest.mark.parametrize("D", [[-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05], [-0.3], [0.1, -0.05, 1e-3, -2e-3, 0.01, 0.02, -0.01, 0.003]],
                         ids=["radtan4", "k1", "rational8"])
def test_init_undistort_rectify_map_against_a_scalar_loop(D):
    w, h = 61, 47
    K = [[458.654 / 12, 0.0, 30.2], [0.0, 457.296 / 12, 22.9], [0.0, 0.0, 1.0]]
    R = _rodrigues(0.004, -0.011, 0.0172).tolist()
    P = [[36.5, 0.0, 31.0, -4.0], [0.0, 36.5, 23.5, 0.0], [0.0, 0.0, 1.0, 0.0]]
    mx, my = rectify.init_undistort_rectify_map(K, D, R, P, w, h)
    sx, sy = _scalar_maps(K, D, R, P, w, h)
    assert mx.dtype == np.float32 and mx.shape == (h, w) and my.shape == (h, w)
    assert np.array_equal(mx.view(np.uint32), sx.view(np.uint32)) and np.array_equal(my.view(np.uint32), sy.view(np.uint32))
    assert np.abs(mx - np.arange(w)).max() > 0.5, "the calibration bends the image"


@pytest.mark.parametrize("K", [[[300.0, 0, 239.5], [0, 300.0, 79.5], [0, 0, 1]], [[718.856, 0, 607.1928], [0, 718.856, 185.2157], [0, 0, 1]]],
                         ids=["small_world", "kitti"])
def test_no_distortion_is_the_identity_grid_exactly(K):
    w, h = 130, 50
    for R, P, D in ((None, None, None), (np.eye(3), K, np.zeros(5)), (np.eye(3), np.hstack([np.array(K), [[-386.1], [0], [0]]]), [0.0] * 8)):
        mx, my = rectify.init_undistort_rectify_map(K, D, R, P, w, h)
        assert np.array_equal(mx, np.tile(np.arange(w, dtype=np.float32), (h, 1)))
        assert np.array_equal(my, np.tile(np.arange(h, dtype=np.float32)[:, None], (1, w)))
    with pytest.raises(ValueError):
        rectify.init_undistort_rectify_map(K, [0.0] * 9, None, None, w, h)


YAML = """%YAML:1.0
Camera.fx: 435.2
Camera.fy: 435.2
Camera.cx: 367.45
Camera.cy: 252.2
Camera.bf: 47.9
LEFT.height: 480
LEFT.width: 752
LEFT.D: !!opencv-matrix
   rows: 1
   cols: 5
   dt: d
   data:[-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.0]
LEFT.K: !!opencv-matrix
   rows: 3
   cols: 3
   dt: d
   data: [458.654, 0.0, 367.215, 0.0, 457.296, 248.375, 0.0, 0.0, 1.0]
LEFT.R:  !!opencv-matrix
   rows: 3
   cols: 3
   dt: d
   data: [0.999966347530033, -0.001422739138722922, 0.008079580483432283, 0.001365741834644127, 0.9999741760894847,
          0.007055629199258132, -0.008089410156878961, -0.007044357138835809, 0.9999424675829176]
LEFT.P:  !!opencv-matrix
   rows: 3
   cols: 4
   dt: d
   data: [435.2046959714599, 0, 367.4517211914062, 0,  0, 435.2046959714599, 252.2008514404297, 0,  0, 0, 1, 0]
RIGHT.D: !!opencv-matrix
   rows: 1
   cols: 5
   dt: d
   data:[-0.28368365, 0.07451284, -0.00010473, -3.555907e-05, 0.0]
RIGHT.K: !!opencv-matrix
   rows: 3
   cols: 3
   dt: d
   data: [457.587, 0.0, 379.999, 0.0, 456.134, 255.238, 0.0, 0.0, 1]
RIGHT.R:  !!opencv-matrix
   rows: 3
   cols: 3
   dt: d
   data: [0.9999633526194376, -0.003625811871560086, 0.007755443660172947, 0.003680398547259526, 0.9999684752771629,
          -0.007035845251224894, -0.007729688520722713, 0.007064130529506649, 0.999945173484644]
RIGHT.P:  !!opencv-matrix
   rows: 3
   cols: 4
   dt: d
   data: [435.2046959714599, 0, 367.4517211914062, -47.90639384423901, 0, 435.2046959714599, 252.2008514404297, 0, 0, 0, 1, 0]
"""


def test_run_cli_reads_the_stereo_calibration_layout(tmp_path):
    path = tmp_path / "stereo.yaml"
    path.write_text(YAML)
    cal = run.read_calibration(str(path))
    assert cal["fx"] == float(np.float32(435.2)) and cal["bf"] == float(np.float32(47.9))   # Camera.* still defines the projections
    left, right = run.read_rectification(str(path))
    assert left["K"].shape == (3, 3) and left["D"].shape == (1, 5) and left["R"].shape == (3, 3) and left["P"].shape == (3, 4)
    assert left["K"][0, 2] == 367.215 and left["R"][1, 2] == 0.007055629199258132 and right["P"][0, 3] == -47.90639384423901
    assert right["D"][0, 2] == -0.00010473
    (mxl, myl), (mxr, myr) = rectify.stereo_maps(left, right, 64, 48)
    assert mxl.shape == (48, 64) and mxr.dtype == np.float32 and not np.array_equal(mxl, mxr)
    # without the keys nothing changes
    plain = tmp_path / "plain.yaml"
    plain.write_text("\n".join(l for l in YAML.splitlines()[:6]) + "\n")
    assert run.read_rectification(str(plain)) is None and run.read_calibration(str(plain)) == cal
    half = tmp_path / "half.yaml"
    half.write_text(YAML[:YAML.index("RIGHT.P")])
    assert run.read_rectification(str(half)) is None
