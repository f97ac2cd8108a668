"""cv::FAST under a mask (include/vo_fast_mask.h) as the tests see it: the expected side composed from the references the suite already
has -- oracle.fast_detect (cv::FAST on the unmasked image), KeyPointsFilter::runByPixelsMask restated in numpy,
corners_mask_cases.ref_disc_mask (the disc mask of vo_corners_mask.h), appendNewFeatures' list rule and the oracle's bucketingFeatures
--, the product's kernels through the coroutine emulator (tests/host_check/fast_mask_emu.cpp), and the images and carried sets
test_fast_mask_ref.py, test_fast_mask_emulation.py and test_gpu_fast_mask.py share: the suite's small_world (480 x 160, seed 11) and
crops of its L[0].

The library loaded into python is built WITHOUT sanitizer flags.  The sanitizer tier is the same harness as a STAND-ALONE program with
its own main(), built with -fsanitize=address,undefined (runtimes linked statically) and run as a child."""
import ctypes as C

import numpy as np

import corners_mask_cases as cm
import detector_cases as dc
import emu_build
import topup_cases as tc
from conftest import vp

EMPTY = dc.EMPTY
CROP_BIG, CROP_SMALL, CROP_ODD = dc.CROP_BIG, dc.CROP_SMALL, tc.CROP_ODD   # 64 x 48: 72 FAST corners; 32 x 32: 14; 61 x 47
carried_set, world_frames, L0, crop = dc.carried_set, dc.world_frames, tc.L0, tc.crop
FME_COUNTS = 6

_cache = {}


def ref_fast(img, threshold=20, nonmax=True):
    """cv::FAST(img, keypoints, threshold, nonmax) + KeyPoint::convert from the oracle: row-major.  Computed once per (image bytes,
    parameters), shared, read-only"""
    from oracle import oracle as orc
    orc.build()
    img = np.ascontiguousarray(img, np.uint8)
    key = (img.shape, img.tobytes(), int(threshold), bool(nonmax))
    if key not in _cache:
        c = orc.fast_detect(img, threshold, nonmax)
        c.setflags(write=False)
        _cache[key] = c
    return _cache[key]


def run_by_pixels_mask(corners, mask):
    """KeyPointsFilter::runByPixelsMask: a keypoint is dropped iff mask((int)(pt.y + 0.5f), (int)(pt.x + 0.5f)) == 0; order kept"""
    c = np.asarray(corners, np.float32).reshape(-1, 2)
    y = (c[:, 1] + np.float32(0.5)).astype(np.int32)
    x = (c[:, 0] + np.float32(0.5)).astype(np.int32)
    return c[np.asarray(mask)[y, x] != 0]


def ref_masked(img, mask, threshold=20, nonmax=True):
    """FastFeatureDetector::create(threshold, nonmax)->detect(img, keypoints, mask): FAST on the unmasked image, then the filter"""
    return run_by_pixels_mask(ref_fast(img, threshold, nonmax), mask)


def every_nth(img, step=40):
    """every step-th unmasked FAST corner as a carried set with zero ages"""
    pts = np.array(ref_fast(img)[::step], np.float32)
    return pts, np.zeros(len(pts), np.int32)


def ref_topup_corners(img, carried, radius, threshold=20, nonmax=True):
    """the detector call of the frame loop with the record on: under the disc mask of the carried points; with none carried the
    unmasked call"""
    pts = np.ascontiguousarray(carried, np.float32).reshape(-1, 2)
    if len(pts) == 0:
        return ref_fast(img, threshold, nonmax)
    h, w = img.shape
    return ref_masked(img, cm.ref_disc_mask(w, h, pts, radius), threshold, nonmax)


def expected_bucketed(img, carried, ages, radius, redetect_below=2000, bucket_size=0, features_per_bucket=1, threshold=20, nonmax=True):
    """appendNewFeatures with the masked detector call (radius None: the unmasked one) when fewer than redetect_below points are
    carried, then bucketingFeatures: (points, ages, number of new corners)"""
    from oracle import oracle as orc
    orc.build()
    h, w = img.shape
    pts = np.asarray(carried, np.float32).reshape(-1, 2)
    ag = np.asarray(ages, np.int32).reshape(-1)
    n_new = 0
    if len(pts) < redetect_below:
        c = ref_fast(img, threshold, nonmax) if radius is None else ref_topup_corners(img, pts, radius, threshold, nonmax)
        n_new = len(c)
        pts = np.vstack([pts, c])
        ag = np.concatenate([ag, np.zeros(n_new, np.int32)])   # (behind a possibly longer ages vector, quirk B3)
    p, a = orc.bucketing_features(h, w, pts, ag, bucket_size or h // 10, features_per_bucket)
    return p, a, n_new


# ---- the emulator ------------------------------------------------------------------------------------------------------------

def load_emu():
    lib = emu_build.shared("fast_mask_emu")
    lib.fme_filter.argtypes = [C.c_void_p] * 7
    lib.fme_route.argtypes = [C.c_void_p] * 11
    return lib


def _standalone(tmp_path, mode, args, timeout=600):
    exe = emu_build.sanitized_program("fast_mask_emu", "FAST_MASK_EMU_MAIN")
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        for a in args:
            f.write(a.tobytes())
    emu_build.run_clean(exe, [mode, fin, fout], timeout)
    return np.fromfile(fout, np.uint8)


SENTINEL = np.float32(-77.0)


def emu_filter(lists, planes, detect, cap, threads, tmp_path=None):
    """fast_mask_filter_kernel over caller-made lists.  lists: per frame (points (k, 2), count the kernel is told -- it may exceed cap);
    planes (n, h, pitch) uint8 whose first pitch - 3 columns are the mask and whose last 3 are padding (the harness gives every plane
    a block that ends with the last mask byte); detect: per-frame flags.
    Returns (out (n, cap, 2) -- SENTINEL where the kernel wrote nothing --, n_out (n,) -- -5 where it wrote nothing).
    tmp_path: through the stand-alone sanitizer program instead"""
    n, h, pitch = planes.shape
    hd = np.array([n, cap, pitch - 3, h, pitch, threads], np.int32)
    pin = np.zeros((n, cap, 2), np.float32)
    nin = np.zeros(n, np.int32)
    for f, (p, count) in enumerate(lists):
        p = np.asarray(p, np.float32).reshape(-1, 2)
        pin[f, :len(p)] = p
        nin[f] = count
    det = np.asarray(detect, np.int32)
    out = np.full((n, cap, 2), SENTINEL, np.float32)
    nout = np.full(n, -5, np.int32)
    planes = np.ascontiguousarray(planes, np.uint8)
    if tmp_path is None:
        assert load_emu().fme_filter(vp(hd), vp(pin), vp(nin), vp(planes), vp(det), vp(out), vp(nout)) == 0
        return out, nout
    raw = _standalone(tmp_path, "filter", (hd, pin, nin, planes, det, out, nout))
    return raw[:8 * n * cap].view(np.float32).reshape(n, cap, 2).copy(), raw[8 * n * cap:].view(np.int32).copy()


def _route_args(imgs, frames, radius, lcap, bucket_size, fpb, bucket_threads, out_cap, redetect_below, lookahead, filter_threads, threshold, nonmax):
    h, w = imgs[0].shape
    lcap = w * h if lcap is None else lcap
    out_cap = lcap if out_cap is None else out_cap
    n = len(frames)
    hd = np.array([len(imgs), w, h, n, threshold, int(nonmax), lcap, bucket_size or h // 10, fpb, bucket_threads, out_cap, redetect_below, int(lookahead),
                   int(radius), filter_threads, 0], np.int32)
    quad_l0 = np.array([f[0] for f in frames], np.int32)
    nt = np.array([len(f[1]) for f in frames], np.int32)
    carried = np.zeros((n, lcap, 2), np.float32)
    ages = np.zeros((n, lcap), np.int32)
    for i, (_, p, a) in enumerate(frames):
        carried[i, :len(p)] = p
        ages[i, :len(a)] = a
    buf = np.stack([np.ascontiguousarray(i, np.uint8) for i in imgs])
    return (hd, quad_l0, nt, carried, ages, buf), (n, h, w, lcap, out_cap)


def _route_unpack(counts, pts, ages, planes, new, n):
    names = ("n", "overflow", "n_new", "n_raw", "detect", "plane_touched")
    out = []
    for f in range(n):
        d = {k: int(counts[i, f]) for i, k in enumerate(names)}
        d.update(pts=pts[f, :max(0, d["n"])].copy(), ages=ages[f, :max(0, d["n"])].copy(), plane=planes[f].copy(),
                 new=new[f, :max(0, min(d["n_new"], new.shape[1]))].copy())
        out.append(d)
    return out


def emu_route(imgs, frames, radius=5, lcap=None, bucket_size=0, fpb=1, bucket_threads=1024, out_cap=None, redetect_below=2000, lookahead=False,
              filter_threads=1024, threshold=20, nonmax=True, tmp_path=None):
    """imgs: the image table (equal shapes); frames: [(table image of the frame's left t0 image, carried points, ages)].  One emulated
    run of the step's detection with the record on.  Per frame a dict: pts, ages, n (bucketed), overflow, n_new, n_raw, detect,
    plane_touched, plane, new (the masked list).  tmp_path: through the stand-alone sanitizer program instead"""
    args, (n, h, w, lcap, out_cap) = _route_args(imgs, frames, radius, lcap, bucket_size, fpb, bucket_threads, out_cap, redetect_below, lookahead,
                                                 filter_threads, threshold, nonmax)
    if tmp_path is None:
        counts = np.zeros((FME_COUNTS, n), np.int32)
        pts, ages = np.zeros((n, out_cap, 2), np.float32), np.zeros((n, out_cap), np.int32)
        planes = np.zeros((n, h, w), np.uint8)
        new = np.zeros((n, lcap, 2), np.float32)
        assert load_emu().fme_route(*[vp(a) for a in args], vp(counts), vp(pts), vp(ages), vp(planes), vp(new)) == 0
        return _route_unpack(counts, pts, ages, planes, new, n)
    raw = _standalone(tmp_path, "route", args)
    o = np.cumsum([0, 4 * FME_COUNTS * n, 8 * n * out_cap, 4 * n * out_cap, n * h * w, 8 * n * lcap])
    assert len(raw) == o[-1]
    return _route_unpack(raw[o[0]:o[1]].view(np.int32).reshape(FME_COUNTS, n), raw[o[1]:o[2]].view(np.float32).reshape(n, out_cap, 2),
                         raw[o[2]:o[3]].view(np.int32).reshape(n, out_cap), raw[o[3]:o[4]].reshape(n, h, w),
                         raw[o[4]:o[5]].view(np.float32).reshape(n, lcap, 2), n)
