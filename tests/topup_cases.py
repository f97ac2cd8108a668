"""The frame loop's top-up under a mask of the carried points (include/vo_topup.h) as the tests see it: the expected side composed from
the references the suite already has -- corners_mask_cases.ref_disc_mask (the header's disc mask), corners_response_cases.ref_detect
(tests/host_check/corners_response_ref.c: goodFeaturesToTrack with its mask argument), appendNewFeatures' list rule and the oracle's
bucketingFeatures --, the product's kernels through the coroutine emulator (tests/host_check/topup_emu.cpp), and the images and carried
sets test_topup_ref.py, test_topup_emulation.py and test_gpu_topup.py share: the suite's small_world (480 x 160, seed 11) and crops
of its L[0].

The library loaded into python is built WITHOUT sanitizer flags.  The sanitizer tier is the same harness as a STAND-ALONE program with
its own main(), built with -fsanitize=address,undefined (runtimes linked statically) and run as a child."""
import ctypes as C

import numpy as np

import corners_emu as ce
import corners_mask_cases as cm
import corners_response_cases as crc
import detector_cases as dc
import emu_build
from conftest import vp

DEFAULT, HARRIS5, EMPTY = dc.DEFAULT, dc.HARRIS5, dc.EMPTY
CROP_BIG, CROP_SMALL = dc.CROP_BIG, dc.CROP_SMALL
CROP_ODD = (slice(40, 87), slice(100, 161))     # 61 x 47: w h is odd, so the second frame's map starts off the 16-byte grid
carried_set, world_frames = dc.carried_set, dc.world_frames
TE_COUNTS = 10

_cache = {}


def L0():
    return world_frames()[1][0]


def crop(which, frame=0):
    return np.ascontiguousarray(world_frames()[1][frame][which])


def ref_masked(img, mask, det=DEFAULT):
    """cv::goodFeaturesToTrack(img, ..., mask, block_size, use_harris, k) from corners_response_ref.c: the corners in the call's order"""
    return crc.ref_detect(np.ascontiguousarray(img, np.uint8), mask, det["max_corners"], det["quality_level"], det["min_distance"], det["block_size"],
                          int(bool(det["use_harris"])), det["k"])[0]


def ref_topup_corners(img, carried, radius, det=DEFAULT):
    """the top-up's detector call: under the disc mask of the carried points; with none carried the unmasked call of vo_detector.h.
    Computed once per (image bytes, carried bytes, radius, parameters), shared, read-only"""
    img = np.ascontiguousarray(img, np.uint8)
    pts = np.ascontiguousarray(carried, np.float32).reshape(-1, 2)
    if len(pts) == 0:
        return dc.ref_corners(img, **det)
    key = (img.shape, img.tobytes(), pts.tobytes(), int(radius), tuple(sorted(det.items())))
    if key not in _cache:
        h, w = img.shape
        c = ref_masked(img, cm.ref_disc_mask(w, h, pts, radius), det)
        c.setflags(write=False)
        _cache[key] = c
    return _cache[key]


def strongest(img, n, det=DEFAULT):
    """the n strongest unmasked corners (goodFeaturesToTrack's order is by descending quality)"""
    return np.array(dc.ref_corners(img, **det)[:n], np.float32)


def filtered_afterwards(img, carried, radius, det=DEFAULT):
    """the WRONG reading: detect unmasked, drop the corners under the mask"""
    h, w = img.shape
    m = cm.ref_disc_mask(w, h, carried, radius)
    c = dc.ref_corners(img, **det)
    return c[m[c[:, 1].astype(int), c[:, 0].astype(int)] != 0]


def expected_bucketed(img, carried, ages, radius, det=DEFAULT, redetect_below=2000, bucket_size=0, features_per_bucket=1):
    """appendNewFeatures with the masked detector call when fewer than redetect_below points are carried, then bucketingFeatures:
    (points, ages, number of new corners)"""
    from oracle import oracle as orc
    orc.build()
    h, w = img.shape
    pts = np.asarray(carried, np.float32).reshape(-1, 2)
    ag = np.asarray(ages, np.int32).reshape(-1)
    n_new = 0
    if len(pts) < redetect_below:
        c = ref_topup_corners(img, pts, radius, det)
        n_new = len(c)
        pts = np.vstack([pts, c])
        ag = np.concatenate([ag, np.zeros(n_new, np.int32)])
    p, a = orc.bucketing_features(h, w, pts, ag, bucket_size or h // 10, features_per_bucket)
    return p, a, n_new


# ---- the emulator ------------------------------------------------------------------------------------------------------------

def load_emu():
    lib = emu_build.shared("topup_emu")
    lib.te_run.argtypes = [C.c_void_p] * 11
    return lib


def _pack(imgs, frames, radius, det, lcap, bucket_size, fpb, bucket_threads, out_cap, redetect_below, lookahead, stride):
    h, w = imgs[0].shape
    stride = w if stride is None else stride
    n = len(frames)
    hd = np.array([len(imgs), w, h, stride, n, det["max_corners"], det["block_size"], int(det["use_harris"]), lcap, bucket_size or h // 10, fpb,
                   bucket_threads, out_cap, redetect_below, int(lookahead), int(radius)], np.int32)
    q = np.array([det["quality_level"], det["min_distance"], det["k"]], np.float64)
    quad_l0 = np.array([f[0] for f in frames], np.int32)
    nt = np.array([len(f[1]) for f in frames], np.int32)
    carried = np.zeros((n, lcap, 2), np.float32)
    ages = np.zeros((n, lcap), np.int32)
    for i, (_, p, a) in enumerate(frames):
        carried[i, :len(p)] = p
        ages[i, :len(a)] = a
    buf = np.stack([ce.strided(i, stride) for i in imgs])
    return hd, q, quad_l0, nt, carried, ages, buf


def _unpack(counts, pts, ages, planes, n):
    names = ("n", "overflow", "n_new", "n_cand", "map_touched", "detect", "cand_touched", "plane_touched")
    out = []
    for f in range(n):
        d = {k: int(counts[i, f]) for i, k in enumerate(names)}
        d.update(pts=pts[f, :max(0, d["n"])].copy(), ages=ages[f, :max(0, d["n"])].copy(), plane=planes[f].copy(),
                 max_key=int(counts[8, f]) & 0xffffffff, body_key=int(counts[9, f]) & 0xffffffff)
        out.append(d)
    return out


def _sizes(imgs, lcap, out_cap):
    h, w = imgs[0].shape
    lcap = w * h if lcap is None else lcap
    return h, w, lcap, lcap if out_cap is None else out_cap


def emu_run(imgs, frames, radius=5, det=DEFAULT, lcap=None, bucket_size=0, fpb=1, bucket_threads=1024, out_cap=None, redetect_below=2000, lookahead=False,
            stride=None):
    """imgs: the image table (equal shapes); frames: [(table image of the frame's left t0 image, carried points, ages)].  One emulated
    run of the step's detection with the top-up on.  Per frame a dict: pts, ages, n (bucketed), overflow, n_new, n_cand, detect,
    map_touched, cand_touched, plane_touched, plane, max_key (corn_max_frames_kernel's), body_key (corn_map_body's under the plane)"""
    h, w, lcap, out_cap = _sizes(imgs, lcap, out_cap)
    args = _pack(imgs, frames, radius, det, lcap, bucket_size, fpb, bucket_threads, out_cap, redetect_below, lookahead, stride)
    n = len(frames)
    counts = np.zeros((TE_COUNTS, n), np.int32)
    pts, ages = np.zeros((n, out_cap, 2), np.float32), np.zeros((n, out_cap), np.int32)
    planes = np.zeros((n, h, w), np.uint8)
    assert load_emu().te_run(*[vp(a) for a in args], vp(counts), vp(pts), vp(ages), vp(planes)) == 0
    return _unpack(counts, pts, ages, planes, n)


def run_standalone(tmp_path, imgs, frames, radius=5, det=DEFAULT, lcap=None, bucket_size=0, fpb=1, bucket_threads=1024, out_cap=None, redetect_below=2000,
                   lookahead=False, stride=None):
    """emu_run through the stand-alone ASan + UBSan program, run as a child: no report, exit status 0"""
    exe = emu_build.sanitized_program("topup_emu", "TOPUP_EMU_MAIN")
    h, w, lcap, out_cap = _sizes(imgs, lcap, out_cap)
    args = _pack(imgs, frames, radius, det, lcap, bucket_size, fpb, bucket_threads, out_cap, redetect_below, lookahead, stride)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        for a in args:
            f.write(a.tobytes())
    emu_build.run_clean(exe, [fin, fout], 600)
    n = len(frames)
    raw = np.fromfile(fout, np.uint8)
    o0, o1, o2 = 4 * TE_COUNTS * n, 4 * TE_COUNTS * n + 8 * n * out_cap, 4 * TE_COUNTS * n + 12 * n * out_cap
    counts = raw[:o0].view(np.int32).reshape(TE_COUNTS, n)
    pts = raw[o0:o1].view(np.float32).reshape(n, out_cap, 2)
    ages = raw[o1:o2].view(np.int32).reshape(n, out_cap)
    planes = raw[o2:].reshape(n, h, w)
    return _unpack(counts, pts, ages, planes, n)
