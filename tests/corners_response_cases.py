"""The Shi-Tomasi detector with a response (include/vo_corners_response.h: blockSize 3 or 5, minimum eigenvalue or Harris, k) as the
tests see it: the restatement of OpenCV (tests/host_check/corners_response_ref.c, the specification), the product's kernels run
through the coroutine emulator (tests/host_check/corners_response_emu.cpp), the generators and the case table that
test_corners_response_ref.py, test_corners_response_emulation.py and test_gpu_corners_response.py share.

The libraries loaded into python are built WITHOUT sanitizer flags whatever the environment says.  The sanitizer tier is the same
harness as a STAND-ALONE program with its own main(), built with -fsanitize=address,undefined (runtimes linked statically) and run
as a child.  Nothing instrumented is loaded into python."""
import ctypes as C
import functools

import numpy as np

import corners_emu as ce
import emu_build
from conftest import vp

RESPONSES = [(5, 0), (3, 1), (5, 1)]          # (block_size, use_harris) beside (3, 0), which is vo_corners.h's
K = 0.04
CM_COLS5 = 252                                # columns a workgroup of corn_map_resp_kernel<5, *> owns (256 threads, two halo columns a side)
SEAM_WIDTHS = [CM_COLS5 - 1, CM_COLS5, CM_COLS5 + 1, 2 * CM_COLS5]


def load_ref():
    """libcorners_response_ref.so (plain C, -ffp-contract=off), built when stale and loaded once per session"""
    lib = emu_build.shared("corners_response_ref", cc="gcc", flags=["-std=c99", "-ffp-contract=off", "-Wall"], libs=["-lm"])
    lib.crr_map.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_int, C.c_int, C.c_int]
    lib.crr_detect.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_double,
                               C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    return lib


def load_emu():
    lib = emu_build.shared("corners_response_emu")
    lib.cre_map.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p]
    lib.cre_detect.argtypes = [C.c_void_p] * 3 + [C.c_int] * 9 + [C.c_double, C.c_double, C.c_int, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_int,
                                                                  C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


# ---- the reference -----------------------------------------------------------------------------------------------------------

def ref_map(img, block=3, harris=0, k=K, trap=0, order=0, form=0, stride=None):
    h, w = img.shape
    buf = np.ascontiguousarray(img) if stride is None else ce.strided(img, stride)
    out = np.zeros((h, w), np.float32)
    assert load_ref().crr_map(vp(buf), w, h, buf.shape[1], block, harris, k, vp(out), trap, order, form) == 0
    return out


def ref_detect(img, mask=None, max_corners=0, quality_level=0.01, min_distance=5.0, block=3, harris=0, k=K, cap=None, trap=0):
    """(corners [min(n, cap), 2], n found, candidates) of cv::goodFeaturesToTrack(img, ..., mask, block, harris, k)"""
    h, w = img.shape
    buf = np.ascontiguousarray(img)
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    cap = w * h if cap is None else cap
    pts = np.zeros((max(cap, 1), 2), np.float32)
    nc = C.c_int(0)
    n = load_ref().crr_detect(vp(buf), w, h, w, None if m is None else vp(m), w, max_corners, quality_level, min_distance, block, harris, k, vp(pts),
                              cap, C.byref(nc), trap)
    assert n >= 0
    return pts[:min(n, cap)].copy(), n, nc.value


# ---- the emulator ------------------------------------------------------------------------------------------------------------

def emu_map(img, block, harris, k=K, stride=None):
    h, w = img.shape
    buf = ce.strided(img, w if stride is None else stride)
    out = np.zeros((h, w), np.float32)
    assert load_emu().cre_map(vp(buf), w, h, buf.shape[1], block, harris, k, vp(out)) == 0
    return out


def _pack(imgs, masks, stride, mask_stride):
    h, w = imgs[0].shape
    buf = np.stack([ce.strided(i, stride) for i in imgs])
    use = masks is not None
    masks = [None] * len(imgs) if masks is None else masks
    on = np.array([m is not None for m in masks], np.uint8)
    mbuf = np.stack([ce.strided(np.zeros((h, w), np.uint8) if m is None else m, mask_stride) for m in masks])
    return buf, mbuf, on, int(use)


def emu_detect(imgs, masks, max_corners, quality_level, min_distance, block, harris, k=K, cap=None, lcap=None, stride=None, mask_stride=None, first=0,
               n=None):
    """images (a list of equal shape) with their masks (None: no mask table; an entry None: that image has none) through one
    emulated run over images first .. first + n - 1.  Returns per image of the run (corners, n found or -1, candidates, map)"""
    h, w = imgs[0].shape
    stride = w if stride is None else stride
    mask_stride = w if mask_stride is None else mask_stride
    buf, mbuf, on, use = _pack(imgs, masks, stride, mask_stride)
    n = len(imgs) - first if n is None else n
    cap = w * h if cap is None else cap
    lcap = w * h if lcap is None else lcap
    pts = np.zeros((n, max(cap, 1), 2), np.float32)
    nout, ncand = np.zeros(n, np.int32), np.zeros(n, np.int32)
    maps = np.zeros((n, h, w), np.float32)
    rc = load_emu().cre_detect(vp(buf), vp(mbuf), vp(on), use, len(imgs), first, n, w, h, stride, mask_stride, max_corners, quality_level, min_distance,
                               block, harris, k, lcap, vp(pts), cap, vp(nout), vp(ncand), vp(maps))
    assert rc == 0
    return [(pts[s, :max(0, min(int(nout[s]), cap))].copy(), int(nout[s]), int(ncand[s]), maps[s]) for s in range(n)]


def run_standalone(tmp_path, imgs, masks, max_corners, quality_level, min_distance, block, harris, k, cap, lcap, stride, mask_stride):
    """the images and masks through the stand-alone ASan + UBSan program, run as a child: no report, exit status 0.  Returns
    (cre_map of image 0, [(corners, n, candidates, map)])"""
    exe = emu_build.sanitized_program("corners_response_emu", "CORNERS_RESPONSE_EMU_MAIN")
    h, w = imgs[0].shape
    n = len(imgs)
    buf, mbuf, on, use = _pack(imgs, masks, stride, mask_stride)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([n, w, h, stride, mask_stride, use, max_corners, lcap, cap, block, harris], np.int32).tobytes())
        f.write(np.array([quality_level, min_distance, k], np.float64).tobytes())
        f.write(buf.tobytes() + mbuf.tobytes() + on.tobytes())
    emu_build.run_clean(exe, [fin, fout], 600)
    raw = np.fromfile(fout, np.uint8)
    o = 4 * w * h
    one = raw[:o].view(np.float32).reshape(h, w)
    cnt = raw[o:o + 8 * n].view(np.int32).reshape(2, n)
    o += 8 * n
    pts = raw[o:o + 8 * n * cap].view(np.float32).reshape(n, cap, 2)
    o += 8 * n * cap
    maps = raw[o:].view(np.float32).reshape(n, h, w)
    return one, [(pts[s, :max(0, min(int(cnt[0, s]), cap))].copy(), int(cnt[0, s]), int(cnt[1, s]), maps[s]) for s in range(n)]


# ---- images and the case table -----------------------------------------------------------------------------------------------

def ramp(w, h):
    """img[y, x] = 4 x, clipped at 252: no vertical gradient, so a * c - b * b = 0 and the Harris map is -k a^2 <= 0 -- negative over
    the ramp (32 x 32: everywhere).  THE NEGATIVE MAXIMUM: at quality_level 0.01 the threshold (float)(max * q) lies above every value
    (no corners); at 3 it lies below them and the negative plateau yields hundreds of candidates"""
    return np.tile(np.minimum(4 * np.arange(w), 252).astype(np.uint8), (h, 1))


def one_sided(w, h, seed):
    """noise with a dark left half-border and a bright right one: the box sum's border samples carry a one-sided gradient, where
    cov of the reflected SOURCE has the wrong sign of dx dy (the trap)"""
    img = ce.noise(w, h, seed)
    img[:, 0] = 0
    img[:, -1] = 255
    return img


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


CONTENTS = [("noise", lambda w, h: ce.noise(w, h, 41)), ("blobs", lambda w, h: ce.blobs(w, h, 42)), ("squares", lambda w, h: ce.squares(w, h, 43)),
            ("periodic", lambda w, h: ce.periodic(w, h)), ("border_max", ce.border_max), ("dark_highlights", lambda w, h: ce.dark_highlights(w, h, 44))]
DISTANCES = [0.0, 1.0, 5.0, 10.5]
RAMP_QUALITIES = [0.01, 3.0]
HARRIS_KS = [0.0, -0.1, 0.25]


@functools.lru_cache(maxsize=None)
def content(name, w, h):
    img = dict(CONTENTS)[name](w, h)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def expected(name, w, h, block, harris, md, k=K, q=0.01, mc=0):
    """the reference's (corners, n, candidates) for a content of the table: computed once, shared, read-only"""
    pts, n, nc = ref_detect(content(name, w, h), None, mc, q, md, block, harris, k)
    pts.setflags(write=False)
    return pts, n, nc


@functools.lru_cache(maxsize=None)
def expected_map(name, w, h, block, harris, k=K):
    m = ref_map(content(name, w, h), block, harris, k)
    m.setflags(write=False)
    return m
