"""The frame loop's detector (include/vo_detector.h) as the tests see it: the expected side -- goodFeaturesToTrack from the references
(the reference's own featureDetectionGoodFeaturesToTrack where oracle/_ref exists and the parameters are its literals, else
tests/host_check/corners_ref.c / corners_response_ref.c), appendNewFeatures' list rule and the oracle's bucketingFeatures -- the
product's frames-form kernels + bucket_kernel through the coroutine emulator (tests/host_check/detector_emu.cpp), and the images and
carried sets test_detector_ref.py, test_detector_emulation.py and test_gpu_detector.py share.

The library loaded into python is built WITHOUT sanitizer flags.  The sanitizer tier is the same harness as a STAND-ALONE program with
its own main(), built with -fsanitize=address,undefined (runtimes linked statically) and run as a child."""
import ctypes as C
import functools

import numpy as np

import corners_emu as ce
import corners_response_cases as crc
import emu_build
from conftest import vp

DEFAULT = dict(max_corners=5000, quality_level=0.01, min_distance=5.0, block_size=3, use_harris=False, k=0.04)  # feature.cpp:53-61
HARRIS5 = dict(DEFAULT, block_size=5, use_harris=True)
FEW = dict(DEFAULT, max_corners=50, quality_level=0.05, min_distance=10.0)
CROP_BIG, CROP_SMALL = (slice(40, 88), slice(100, 164)), (slice(40, 72), slice(100, 132))   # 64 x 48: 58 corners; 32 x 32: 19


@functools.lru_cache(maxsize=None)
def world_frames(n=5):
    """the suite's small_world (conftest.py: 480 x 160, seed 11): n stereo frames, rendered once"""
    from visual_odom_amd import synth
    world = synth.StereoWorld(seed=11, width=480, height=160, fx=300.0, cx=239.5, cy=79.5, bf=-160.0, tex_size=1024)
    lefts, rights, _, _ = world.render_sequence(n)
    for a in list(lefts) + list(rights):
        a.setflags(write=False)
    return world, lefts, rights


_corner_cache = {}


def ref_corners(img, max_corners=5000, quality_level=0.01, min_distance=5.0, block_size=3, use_harris=False, k=0.04):
    """cv::goodFeaturesToTrack(img, ..., noArray(), block_size, use_harris, k) from the references: the corners in the call's own
    order.  Computed once per (image bytes, parameters), shared, read-only"""
    img = np.ascontiguousarray(img, np.uint8)
    key = (img.shape, img.tobytes(), max_corners, quality_level, min_distance, block_size, bool(use_harris), k)
    if key not in _corner_cache:
        if (block_size, bool(use_harris)) == (3, False):
            pts = ce.ref_detect(img, max_corners, quality_level, min_distance)[0]
            from oracle import oracle as orc
            if (max_corners, quality_level, min_distance) == (5000, 0.01, 5.0) and orc.ref_lib() is not None:
                own = orc.ref_feature_detection_gftt(img)[0]   # the reference's own function, its literals
                assert np.array_equal(own, pts)
        else:
            pts = crc.ref_detect(img, None, max_corners, quality_level, min_distance, block_size, int(bool(use_harris)), k)[0]
        pts.setflags(write=False)
        _corner_cache[key] = pts
    return _corner_cache[key]


def expected_bucketed(img, carried, ages, det=DEFAULT, redetect_below=2000, bucket_size=0, features_per_bucket=1):
    """appendNewFeatures with the one detector call swapped (feature.cpp:255-262) when fewer than redetect_below points are
    carried, then bucketingFeatures: (points, ages, number of new corners)"""
    from oracle import oracle as orc
    orc.build()
    h, w = img.shape
    pts = np.asarray(carried, np.float32).reshape(-1, 2)
    ag = np.asarray(ages, np.int32).reshape(-1)
    n_new = 0
    if len(pts) < redetect_below:
        c = ref_corners(img, **det)
        n_new = len(c)
        pts = np.vstack([pts, c])
        ag = np.concatenate([ag, np.zeros(n_new, np.int32)])   # (ages.insert(ages.end(), n, 0): behind a longer ages vector, quirk B3)
    p, a = orc.bucketing_features(h, w, pts, ag, bucket_size or h // 10, features_per_bucket)
    return p, a, n_new


def carried_set(w, h, n=40, surplus=5, seed=3):
    """n carried points inside the image with ages 0 .. 12 (ages >= 10 are ignored by the buckets) and `surplus` more ages than points"""
    rng = np.random.default_rng(seed)
    pts = np.stack([rng.uniform(0, w - 1, n), rng.uniform(0, h - 1, n)], 1).astype(np.float32)
    ages = (np.arange(n + surplus) % 13).astype(np.int32)
    return pts, ages


EMPTY = (np.zeros((0, 2), np.float32), np.zeros(0, np.int32))


# ---- the emulator ------------------------------------------------------------------------------------------------------------

def load_emu():
    lib = emu_build.shared("detector_emu")
    lib.de_run.argtypes = [C.c_void_p] * 10
    return lib


def _pack(imgs, frames, det, lcap, bucket_size, fpb, bucket_threads, out_cap, redetect_below, lookahead, stride):
    h, w = imgs[0].shape
    stride = w if stride is None else stride
    n = len(frames)
    hd = np.array([len(imgs), w, h, stride, n, det["max_corners"], det["block_size"], int(det["use_harris"]), lcap, bucket_size or h // 10, fpb,
                   bucket_threads, out_cap, redetect_below, int(lookahead), 0], np.int32)
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


def _unpack(counts, pts, ages, n):
    return [dict(pts=pts[f, :max(0, counts[0, f])].copy(), ages=ages[f, :max(0, counts[0, f])].copy(), n=int(counts[0, f]), overflow=int(counts[1, f]),
                 n_new=int(counts[2, f]), n_cand=int(counts[3, f]), touched=int(counts[4, f]), detect=int(counts[5, f])) for f in range(n)]


def emu_run(imgs, frames, det=DEFAULT, lcap=None, bucket_size=0, fpb=1, bucket_threads=1024, out_cap=None, redetect_below=2000, lookahead=False,
            stride=None):
    """imgs: the image table (equal shapes); frames: [(table image of the frame's left t0 image, carried points, ages)].  One emulated
    run of the step's detection.  Per frame a dict: pts, ages, n (bucketed), overflow, n_new, n_cand, touched, detect"""
    h, w = imgs[0].shape
    lcap = w * h if lcap is None else lcap
    out_cap = lcap if out_cap is None else out_cap
    args = _pack(imgs, frames, det, lcap, bucket_size, fpb, bucket_threads, out_cap, redetect_below, lookahead, stride)
    n = len(frames)
    counts = np.zeros((6, n), np.int32)
    pts, ages = np.zeros((n, out_cap, 2), np.float32), np.zeros((n, out_cap), np.int32)
    assert load_emu().de_run(*[vp(a) for a in args], vp(counts), vp(pts), vp(ages)) == 0
    return _unpack(counts, pts, ages, n)


def run_standalone(tmp_path, imgs, frames, det=DEFAULT, lcap=None, bucket_size=0, fpb=1, bucket_threads=1024, out_cap=None, redetect_below=2000,
                   lookahead=False, stride=None):
    """emu_run through the stand-alone ASan + UBSan program, run as a child: no report, exit status 0"""
    exe = emu_build.sanitized_program("detector_emu", "DETECTOR_EMU_MAIN")
    h, w = imgs[0].shape
    lcap = w * h if lcap is None else lcap
    out_cap = lcap if out_cap is None else out_cap
    args = _pack(imgs, frames, det, lcap, bucket_size, fpb, bucket_threads, out_cap, redetect_below, lookahead, stride)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        for a in args:
            f.write(a.tobytes())
    emu_build.run_clean(exe, [fin, fout], 600)
    n = len(frames)
    raw = np.fromfile(fout, np.uint8)
    counts = raw[:24 * n].view(np.int32).reshape(6, n)
    pts = raw[24 * n:24 * n + 8 * n * out_cap].view(np.float32).reshape(n, out_cap, 2)
    ages = raw[24 * n + 8 * n * out_cap:].view(np.int32).reshape(n, out_cap)
    return _unpack(counts, pts, ages, n)
