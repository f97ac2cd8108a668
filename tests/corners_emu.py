"""The Shi-Tomasi detector's two CPU sides as the tests use them: the restatement of OpenCV (tests/host_check/corners_ref.c, the
specification) and the product's corners.hip run through the coroutine emulator (tests/host_check/corners_emu.cpp), plus the case
table test_corners_emulation.py and test_gpu_corners.py share.

The libraries loaded into python are built WITHOUT sanitizer flags whatever the environment says.  The sanitizer tier is the same
harness as a STAND-ALONE program with its own main(): every image and list in an exactly sized heap block, built with
-fsanitize=address,undefined (runtimes linked statically) and run as a child.  Nothing instrumented is loaded into python."""
import ctypes as C

import numpy as np

import emu_build
from conftest import vp


def load_ref():
    """libcorners_ref.so (plain C, -ffp-contract=off), built when stale and loaded once per session"""
    lib = emu_build.shared("corners_ref", cc="gcc", flags=["-std=c99", "-ffp-contract=off", "-Wall"], libs=["-lm"])
    lib.cr_min_eigen_map.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int]
    lib.cr_cell.argtypes = [C.c_double]
    lib.cr_detect.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    return lib


def load_emu():
    """libcorners_emu.so: the detector with and without a mask (ce_map, ce_detect; cme_detect, cme_disc for corners_mask_cases.py)"""
    lib = emu_build.shared("corners_emu")
    lib.ce_map.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.ce_detect.argtypes = [C.c_void_p] + [C.c_int] * 7 + [C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.cme_detect.argtypes = [C.c_void_p] * 3 + [C.c_int] * 8 + [C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.cme_disc.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    return lib


def strided(img, stride):
    """(h, stride) uint8 holding img in its first w columns, 0xEE beyond"""
    h, w = img.shape
    out = np.full((h, stride), 0xEE, np.uint8)
    out[:, :w] = img
    return out


def ref_map(img, trap=0, order=0, stride=None):
    h, w = img.shape
    buf = np.ascontiguousarray(img) if stride is None else strided(img, stride)
    eig = np.zeros((h, w), np.float32)
    assert load_ref().cr_min_eigen_map(vp(buf), w, h, buf.shape[1], vp(eig), trap, order) == 0
    return eig


def ref_detect(img, max_corners=0, quality_level=0.01, min_distance=5.0, cap=None, trap=0, stride=None):
    """(corners [min(n, cap), 2], n found, candidates)"""
    h, w = img.shape
    buf = np.ascontiguousarray(img) if stride is None else strided(img, stride)
    cap = w * h if cap is None else cap
    pts = np.zeros((max(cap, 1), 2), np.float32)
    nc = C.c_int(0)
    n = load_ref().cr_detect(vp(buf), w, h, buf.shape[1], max_corners, quality_level, min_distance, vp(pts), cap, C.byref(nc), trap)
    assert n >= 0
    return pts[:min(n, cap)].copy(), n, nc.value


def emu_map(img, stride=None):
    h, w = img.shape
    buf = strided(img, w if stride is None else stride)
    eig = np.zeros((h, w), np.float32)
    assert load_emu().ce_map(vp(buf), w, h, buf.shape[1], vp(eig)) == 0
    return eig


def emu_detect(imgs, max_corners=0, quality_level=0.01, min_distance=5.0, cap=None, lcap=None, stride=None, first=0, n=None):
    """images (a list of equal shape) through one emulated run over images first .. first + n - 1.  Returns per image of the run
    (corners, n found or -1 for an overflowed list, candidates, suppression rounds)"""
    h, w = imgs[0].shape
    stride = w if stride is None else stride
    buf = np.stack([strided(i, stride) for i in imgs])
    n = len(imgs) - first if n is None else n
    cap = w * h if cap is None else cap
    lcap = w * h if lcap is None else lcap
    pts = np.zeros((n, max(cap, 1), 2), np.float32)
    nout, ncand, rounds = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    rc = load_emu().ce_detect(vp(buf), len(imgs), first, n, w, h, stride, max_corners, quality_level, min_distance, lcap, vp(pts), cap, vp(nout),
                              vp(ncand), vp(rounds))
    assert rc == 0
    return [(pts[s, :max(0, min(int(nout[s]), cap))].copy(), int(nout[s]), int(ncand[s]), int(rounds[s])) for s in range(n)]


def run_standalone(tmp_path, imgs, max_corners, quality_level, min_distance, cap, lcap, stride=None):
    """the images through the stand-alone ASan + UBSan program, run as a child: no report, exit status 0.  Returns (map of image 0,
    [(corners, n, candidates, rounds)])"""
    exe = emu_build.sanitized_program("corners_emu", "CORNERS_EMU_MAIN")
    h, w = imgs[0].shape
    stride = w if stride is None else stride
    n = len(imgs)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([n, w, h, stride, max_corners, lcap, cap], np.int32).tobytes())
        f.write(np.array([quality_level, min_distance], np.float64).tobytes())
        f.write(np.stack([strided(i, stride) for i in imgs]).tobytes())
    emu_build.run_clean(exe, [fin, fout], 600)
    raw = np.fromfile(fout, np.uint8)
    eig = raw[:4 * w * h].view(np.float32).reshape(h, w)
    cnt = raw[4 * w * h:4 * w * h + 12 * n].view(np.int32).reshape(3, n)
    pts = raw[4 * w * h + 12 * n:].view(np.float32).reshape(n, cap, 2)
    return eig, [(pts[s, :max(0, min(int(cnt[0, s]), cap))].copy(), int(cnt[0, s]), int(cnt[1, s]), int(cnt[2, s])) for s in range(n)]


# ---- images ------------------------------------------------------------------------------------------------------------------

def noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def blobs(w, h, seed, count=None):
    """smooth bright blobs on a dark ground: a few strong corners, mostly flat"""
    rng = np.random.default_rng(seed)
    img = np.full((h, w), 20.0)
    yy, xx = np.mgrid[0:h, 0:w]
    for _ in range(count or max(3, w * h // 300)):
        cx, cy, a, s = rng.uniform(0, w), rng.uniform(0, h), rng.uniform(40, 220), rng.uniform(1.0, 2.5)
        img += a * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * s * s))
    return np.clip(img, 0, 255).astype(np.uint8)


def squares(w, h, seed):
    """axis-parallel rectangles of random gray: exact plateaus and straight edges"""
    rng = np.random.default_rng(seed)
    img = np.full((h, w), 30, np.uint8)
    for _ in range(max(2, w * h // 400)):
        x, y = int(rng.integers(0, w)), int(rng.integers(0, h))
        img[y:y + int(rng.integers(2, 9)), x:x + int(rng.integers(2, 9))] = rng.integers(0, 256)
    return img


def periodic(w, h, period=8):
    """a lattice of identical dots: every dot has the same neighbourhood, so the qualities tie exactly (the address rule)"""
    img = np.zeros((h, w), np.uint8)
    img[period // 2::period, period // 2::period] = 200
    return img


def border_max(w, h):
    """the strongest structure sits on the image's edge, so the map's maximum is a border pixel -- which is never a candidate, but
    sets the threshold -- over faint interior blobs"""
    img = blobs(w, h, 5).astype(np.int32) // 4 + 10
    img[0, w // 2] = 255
    img[0, w // 2 + 1] = 0
    img[1, w // 2] = 0
    return img.astype(np.uint8)


def dark_highlights(w, h, seed):
    """a dark noisy frame (values 0 .. 5) with a few highlights above a flat area: the f64 operations of boxFilter's running column
    sum are inexact here, and the residual they leave is carried down the column -- about 1e-19 in the flat rows, where a plain
    three-term sum gives 0.  Upstream's summation ORDER is part of the result on this image"""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 6, (h, w)).astype(np.uint8)
    m = rng.random((h, w)) < 0.02
    img[m] = rng.integers(150, 256, int(m.sum()))
    img[(2 * h) // 3:] = 3
    return img


def chain(w, h, count, step=3):
    """a row of dots `step` pixels apart whose brightness falls along the row: with min_distance > step every dot conflicts with its
    better neighbour, so the serial loop's decisions depend on each other along the whole row -- `count` dots deep"""
    img = np.zeros((h, w), np.uint8)
    for k in range(count):
        img[h // 2, 3 + step * k] = 250 - 3 * k
    return img


SHAPES = [(3, 3), (5, 4), (17, 13), (64, 16), (65, 17), (131, 67)]
