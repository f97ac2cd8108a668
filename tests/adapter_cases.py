"""The shipped adapter (adapters/feature_hip.cpp) through the C exports of oracle/ref_dropin/dropin_glue.cpp: featureTracking_hip,
featureDetectionGoodFeaturesToTrack_hip, goodFeaturesToTrack_hip and the process-global state behind them (the kept pair of
vo_adapter_keep_pair, the one context that vo_adapter_context_for destroys and re-creates when a call brings a larger image or more
points).  Expected values come from the CPU libraries alone: the reference's own featureTracking / featureDetectionGoodFeaturesToTrack
/ circularMatching compiled where they lie (oracle/_ref/libvo_refglue.so) and corners_mask_cases.ref_detect.  Everything is
identity -- float bits, bytes, lengths.

Run as a SCRIPT in a fresh child process by tests/test_gpu_adapter.py: the adapter's context belongs to the process, only grows, and
other tests of a session use it too.  Prints one JSON object {"checks": {name: true | false}, "details": {name: text of a false
one}, "inputs": crc of the frames} and exits 0 iff every check holds, 1 (with that line) when one does not, 3 when the script itself failed.  A check whose name starts with "premise" is about the expected
side alone.  Needs a GPU (vo_create)."""
import ctypes as C
import json
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import corners_emu as ce  # noqa: E402
import corners_mask_cases as cm  # noqa: E402
from corners_scale import tiles  # noqa: E402  (the 3 x 3 plateau pattern, shared with the detector's scale cases)
import flow_cases as fc  # noqa: E402
import flow_win_cases as wc  # noqa: E402
from oracle import oracle as orc  # noqa: E402

CV_8UC1, CV_32FC1 = 0, 5
STALE = -7.5               # what the output arrays hold on entry
LIMIT_SHAPE = (640, 480)   # corners 5 pixels apart: 480 x 160 holds fewer than 5000 of them, so the 5000 limit cannot bind there


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def small_seq():
    """tests/conftest.py's small_seq (test_gpu_adapter.py compares the crc with the fixture's)"""
    from visual_odom_amd import synth
    world = synth.StereoWorld(seed=11, width=480, height=160, fx=300.0, cx=239.5, cy=79.5, bf=-160.0, tex_size=1024)
    lefts, rights, _, _ = world.render_sequence(3)
    pts = [np.ascontiguousarray(synth.select_keypoints(lefts[k], bucket=16, per_bucket=2), np.float32) for k in range(2)]
    return dict(L=[np.ascontiguousarray(a, np.uint8) for a in lefts], R=[np.ascontiguousarray(a, np.uint8) for a in rights], pts=pts)


def crc(seq):
    return zlib.crc32(b"".join(a.tobytes() for a in seq["L"] + seq["R"] + seq["pts"]))


def padded(imgs, pad_x=37, pad_y=9, fill=200):
    """views of equal row step != cols into one block (an ROI of a larger cv::Mat), the same pixels"""
    h, w = imgs[0].shape
    big = np.full((len(imgs), h + pad_y, w + pad_x), fill, np.uint8)
    oy, ox = pad_y // 2, pad_x // 3
    big[:, oy:oy + h, ox:ox + w] = np.stack(imgs)
    return [big[i, oy:oy + h, ox:ox + w] for i in range(len(imgs))]


def _img(a):
    """(address, row step in bytes) of an 8-bit image or view -- never a copy: the keep-pair logic compares addresses"""
    assert a.dtype == np.uint8 and a.ndim == 2 and a.strides[1] == 1 and a.strides[0] >= a.shape[1]
    return C.c_void_p(a.ctypes.data), int(a.strides[0])


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


class AdapterError(Exception):
    pass


class Adapter:
    """ctypes over oracle/_ref/libvo_ref_dropin.so's adapter_* exports"""

    def __init__(self):
        self.lib = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libvo_ref_dropin.so"))
        self.lib.adapter_last_error.restype = C.c_char_p
        self.lib.adapter_kept_calls.restype = C.c_long
        self.lib.adapter_gftt.argtypes = [C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] + [C.c_int] * 5 + [C.c_double, C.c_double, C.c_void_p, C.c_int]

    def _rc(self, rc):
        if rc < 0:
            raise AdapterError("%d: %s" % (rc, self.lib.adapter_last_error().decode()))
        return rc

    def keep_pair(self, on):
        self.lib.adapter_keep_pair(int(on))

    def kept_calls(self):
        return int(self.lib.adapter_kept_calls())

    def feature_tracking(self, img1, img2, pts):
        """(points1, points2, status) as featureTracking_hip leaves the three vectors; points2 holds n stale points on entry"""
        (a, step), (b, step_b) = _img(img1), _img(img2)
        assert step == step_b and img1.shape == img2.shape
        h, w = img1.shape
        p1 = np.array(pts, np.float32).reshape(-1, 2).copy()
        n = len(p1)
        p2 = np.full((n + 4, 2), STALE, np.float32)
        st = np.full(n + 4, 9, np.uint8)
        n2, ns = C.c_int(n), C.c_int(-1)
        m = self._rc(self.lib.adapter_feature_tracking(a, b, w, h, step, _vp(p1), n, _vp(p2), C.byref(n2), n + 4, _vp(st), C.byref(ns), n + 4))
        return p1[:m].copy(), p2[:n2.value].copy(), st[:ns.value].copy()

    def gftt_default(self, img, on_entry=0, cap=None):
        """(corners, n) of featureDetectionGoodFeaturesToTrack_hip; `on_entry` stale points are in the vector when it is called"""
        a, step = _img(img)
        h, w = img.shape
        cap = max(5000, on_entry) + 8 if cap is None else cap
        pts = np.full((cap, 2), STALE, np.float32)
        n = self._rc(self.lib.adapter_gftt_default(a, w, h, step, _vp(pts), on_entry, cap))
        return pts[:min(n, cap)].copy(), n

    def gftt(self, img, mask=None, max_corners=0, quality=0.01, min_distance=5.0, img_type=CV_8UC1, mask_type=CV_8UC1, mask_shape=None, cap=None):
        """(corners, n) of goodFeaturesToTrack_hip; mask_shape: the (rows, cols) the mask's header claims (default: its own)"""
        a, step = _img(img)
        h, w = img.shape
        m, mstep = _img(mask) if mask is not None else (None, 0)
        mh, mw = (mask.shape if mask_shape is None else mask_shape) if mask is not None else (0, 0)
        cap = w * h if cap is None else cap
        pts = np.full((cap, 2), STALE, np.float32)
        self.pts = pts   # (a refused call must leave it alone)
        n = self._rc(self.lib.adapter_gftt(a, w, h, step, img_type, m, mstep, mw, mh, mask_type, max_corners, quality, min_distance, _vp(pts), cap))
        return pts[:min(n, cap)].copy(), n

    def circular_matching(self, l0, r0, l1, r1, pts, ages=None):
        """oracle.ref_circular_matching's dict, from circularMatching_hip on these very buffers"""
        ptrs = [_img(a) for a in (l0, r0, l1, r1)]
        assert len({s for _, s in ptrs}) == 1 and len({a.shape for a in (l0, r0, l1, r1)}) == 1
        h, w = l0.shape
        p0 = np.array(pts, np.float32).reshape(-1, 2).copy()
        n = len(p0)
        p1, p2, p3, p0r = (np.full((max(n, 1), 2), STALE, np.float32) for _ in range(4))
        ag = np.zeros(max(n, 1), np.int32) if ages is None else np.array(ages, np.int32).copy()
        na = C.c_int(n if ages is None else len(ag))
        m = self._rc(self.lib.adapter_circular_matching(ptrs[0][0], ptrs[1][0], ptrs[2][0], ptrs[3][0], w, h, ptrs[0][1], _vp(p0), n, _vp(p1),
                                                        _vp(p2), _vp(p3), _vp(p0r), _vp(ag), C.byref(na)))
        return dict(l0=p0[:m].copy(), r0=p1[:m].copy(), r1=p2[:m].copy(), l1=p3[:m].copy(), l0_ret=p0r[:m].copy(), ages=ag[:na.value].copy(), n_out=m)


class Report:
    def __init__(self):
        self.checks, self.details = {}, {}

    def check(self, name, ok, detail=""):
        assert name not in self.checks, name
        self.checks[name] = bool(ok)
        if not ok:
            self.details[name] = str(detail)[:300]
        return bool(ok)

    def guarded(self, name, fn):
        """fn() -> (ok, detail); an exception of the adapter (or a Python one) is the check's failure, not the script's"""
        try:
            ok, detail = fn()
        except Exception as ex:   # noqa: BLE001
            ok, detail = False, "%s: %s" % (type(ex).__name__, ex)
        return self.check(name, ok, detail)


def same_tracking(got, want):
    """points1, points2, status and the three lengths"""
    for k, (g, w) in enumerate(zip(got, want)):
        if len(g) != len(w):
            return False, "length of vector %d: %d, expected %d" % (k, len(g), len(w))
        if g.tobytes() != np.ascontiguousarray(w, g.dtype).tobytes():
            return False, "vector %d differs at %s" % (k, np.flatnonzero((g != w).reshape(len(g), -1).any(1))[:6])
    return True, ""


def same_corners(got, want):
    (gp, gn), (wp, wn) = got, want
    if gn != wn or len(gp) != len(wp):
        return False, "%d corners (%d returned), expected %d" % (gn, len(gp), wn)
    if not np.array_equal(bits(gp), bits(wp)):
        return False, "corners differ from index %d" % int(np.flatnonzero((bits(gp) != bits(wp)).any(1))[0])
    return True, ""


def same_matching(got, want):
    if got["n_out"] != want["n_out"]:
        return False, "%d survivors, expected %d" % (got["n_out"], want["n_out"])
    for k in ("l0", "r0", "r1", "l1", "l0_ret"):
        if not np.array_equal(bits(got[k]), bits(want[k])):
            return False, k
    return (True, "") if np.array_equal(got["ages"], want["ages"]) else (False, "ages")


def main():
    rep, ad = Report(), Adapter()
    seq = small_seq()
    L, R, pts596 = seq["L"], seq["R"], seq["pts"][0]
    crop = lambda a: np.ascontiguousarray(a[:64, :96])   # noqa: E731
    cL, cR = [crop(a) for a in L], [crop(a) for a in R]
    from visual_odom_amd import synth
    crop60 = np.ascontiguousarray(synth.select_keypoints(cL[0], bucket=8, per_bucket=1), np.float32)
    ref_cm = {}

    def want_cm(key, *args):
        if key not in ref_cm:
            ref_cm[key] = orc.ref_circular_matching(*args)
        return ref_cm[key]

    def ref_gftt(img):
        return orc.ref_feature_detection_gftt(np.ascontiguousarray(img), cap=5008)

    # ---- context growth: FIRST, while the process has no context.  96 x 64 -> 480 x 160 (re-created) -> 96 x 64 -> more than 16 384
    # points (re-created) -> circularMatching_hip on the buffers of a pair that an earlier context kept ----
    ad.keep_pair(True)
    kept0 = ad.kept_calls()
    w_a = want_cm("crop01", cL[0], cR[0], cL[1], cR[1], crop60)
    rep.check("premise growth: the 96 x 64 matching keeps and loses points", 10 <= w_a["n_out"] < len(crop60), w_a["n_out"])
    rep.guarded("growth 1: circularMatching_hip at 96 x 64", lambda: same_matching(ad.circular_matching(cL[0], cR[0], cL[1], cR[1], crop60), w_a))
    rep.guarded("growth 2: featureDetectionGoodFeaturesToTrack_hip at 480 x 160", lambda: same_corners(ad.gftt_default(L[0]), ref_gftt(L[0])))
    p_b = w_a["l1"]   # (the reference's loop carries the t1 points on)
    w_b = want_cm("crop12", cL[1], cR[1], cL[2], cR[2], p_b)
    rep.guarded("growth 3: circularMatching_hip at 96 x 64 on the t1 buffers of step 1",
                lambda: same_matching(ad.circular_matching(cL[1], cR[1], cL[2], cR[2], p_b), w_b))
    rep.check("growth 3: not counted as kept (the context of step 1 is gone)", ad.kept_calls() == kept0, ad.kept_calls() - kept0)
    many = wc.lattice(96, 64, 21, step=1.16)
    w_t = orc.ref_feature_tracking(cL[0], cL[1], many)
    rep.check("premise growth: a lattice of more than 16 384 points, tracked and lost ones",
              16384 < len(many) < 17500 and len(w_t[2]) == len(many) and 1000 < len(w_t[0]) < len(many) - 1000, (len(many), len(w_t[0])))
    rep.guarded("growth 4: featureTracking_hip with more than 16 384 points", lambda: same_tracking(ad.feature_tracking(cL[0], cL[1], many), w_t))
    w_c = want_cm("crop20", cL[2], cR[2], cL[0], cR[0], w_b["l1"])
    rep.guarded("growth 5: circularMatching_hip on the t1 buffers of step 3", lambda: same_matching(ad.circular_matching(cL[2], cR[2], cL[0], cR[0], w_b["l1"]), w_c))
    rep.check("growth 5: not counted as kept", ad.kept_calls() == kept0, ad.kept_calls() - kept0)
    ad.keep_pair(False)
    # the context now holds max(16 384, len(many)) points and 480 x 160 pixels (vo_hip.h: the corner-list capacity)
    capacity = max(4 * len(many), 16384, 480 * 160 // 16, LIMIT_SHAPE[0] * LIMIT_SHAPE[1] // 16)

    # ---- featureTracking_hip == the reference's featureTracking ----
    lat = wc.lattice(96, 64, 21)
    for name, a, b, pts in (("L0-L1", L[0], L[1], pts596), ("L0-R0", L[0], R[0], pts596), ("lattice", cL[0], cL[1], lat), ("n = 0", L[0], L[1], pts596[:0])):
        want = orc.ref_feature_tracking(a, b, pts)
        n1, lost = len(want[0]), len(pts) - len(want[0])
        if name.startswith("L0"):
            c = fc.case(name, seq, orc)   # the checker's unfiltered answer, for the premise alone
            left = int(((c["want"][1] == 1) & (c["want"][0] < 0).any(1)).sum())
            rep.check("premise tracking %s: 596 points, tracked, lost, and tracked ones that left the image" % name,
                      len(pts) == 596 and n1 >= 500 and lost >= 20 and (left >= 1 or name == "L0-L1"), (n1, lost, left))
        elif name == "lattice":
            x, y = lat[:, 0], lat[:, 1]
            rep.check("premise tracking lattice: start points on both sides of every border, tracked and lost ones",
                      (x < 0).any() and (x > 96).any() and (y < 0).any() and (y > 64).any() and n1 >= 50 and lost >= 200, (n1, lost))
        rep.guarded("tracking %s" % name, lambda: same_tracking(ad.feature_tracking(a, b, pts), want))
        if name == "L0-R0":
            va, vb = padded([a, b])
            rep.guarded("tracking L0-R0 as views with step != cols", lambda: same_tracking(ad.feature_tracking(va, vb, pts), want))

    # ---- featureDetectionGoodFeaturesToTrack_hip == the reference's featureDetectionGoodFeaturesToTrack ----
    limit_img = ce.noise(LIMIT_SHAPE[0], LIMIT_SHAPE[1], 21)
    for name, img in (("noise 131 x 67", ce.noise(131, 67, 21)), ("blobs 131 x 67", ce.blobs(131, 67, 22)), ("L0", L[0]), ("limit binds", limit_img)):
        want = ref_gftt(img)
        if name == "limit binds":
            unlimited = ce.ref_detect(img, 0, 0.01, 5.0)[1]
            rep.check("premise detection: more than 5000 corners without the limit, 5000 with it", unlimited > 5000 and want[1] == 5000, (unlimited, want[1]))
        else:
            rep.check("premise detection %s: corners, fewer than the limit" % name, 5 <= want[1] < 5000, want[1])
        rep.guarded("detection %s" % name, lambda: same_corners(ad.gftt_default(img), want))
        if name == "noise 131 x 67":
            rep.guarded("detection with a padded step", lambda: same_corners(ad.gftt_default(padded([img], 29, 5)[0]), want))
            rep.guarded("detection into a vector that holds points", lambda: same_corners(ad.gftt_default(img, on_entry=want[1] + 40), want))
            rep.guarded("detection into a vector that holds fewer points", lambda: same_corners(ad.gftt_default(img, on_entry=3), want))

    # ---- goodFeaturesToTrack_hip == corners_mask_cases.ref_detect ----
    def ref_masked(img, mask, mc, q, md):
        p, n, cand = cm.ref_detect(img, mask, max(mc, 0), q, md)   # (maxCorners <= 0: no limit)
        return (p, n), cand

    img = ce.noise(131, 67, 21)
    mask = cm.checker(131, 67)
    want_plain, _ = ref_masked(img, None, 0, 0.01, 5.0)
    want_mask, _ = ref_masked(img, mask, 0, 0.01, 5.0)
    want_17, _ = ref_masked(img, mask, 17, 0.01, 10.5)
    rep.check("premise corners: the mask changes the answer, the limit of 17 binds",
              0 < want_mask[1] < want_plain[1] and not np.array_equal(want_mask[0], want_plain[0][:want_mask[1]]) and want_17[1] == 17
              and ref_masked(img, mask, 0, 0.01, 10.5)[0][1] > 17, (want_plain[1], want_mask[1], want_17[1]))
    rep.guarded("corners without a mask", lambda: same_corners(ad.gftt(img), want_plain))
    rep.guarded("corners under a mask", lambda: same_corners(ad.gftt(img, mask), want_mask))
    rep.guarded("corners under a mask with step != cols", lambda: same_corners(ad.gftt(img, padded([mask], 13, 3, fill=255)[0]), want_mask))
    rep.guarded("corners with image and mask as views", lambda: same_corners(ad.gftt(padded([img], 29, 5)[0], padded([mask], 13, 3, fill=0)[0]), want_mask))
    rep.guarded("corners with maxCorners 17", lambda: same_corners(ad.gftt(img, mask, 17, 0.01, 10.5), want_17))
    # more corners than the adapter's first buffer of 8192 and no limit: the only route to its second vocmask_detect call
    big = tiles(480, 160, cols=120)
    big_mask = cm.checker(480, 160)
    for name, m, mc in (("maxCorners 0", None, 0), ("maxCorners -1 under a mask", big_mask, -1)):
        want, cand = ref_masked(big, m, mc, 0.01, 0.0)
        rep.check("premise corners %s: more than 8192 corners, candidates within the capacity" % name, 8192 < want[1] <= cand <= capacity, (want[1], cand, capacity))
        rep.guarded("corners %s: all of them come back" % name, lambda: same_corners(ad.gftt(big, m, mc, 0.01, 0.0), want))
    flood = tiles(480, 160)
    n_flood = ce.ref_detect(flood, 0, 0.01, 0.0)[2]
    rep.check("premise corners: candidates beyond the capacity", n_flood > capacity, (n_flood, capacity))

    def refused(text, **kw):
        def run():
            try:
                got = ad.gftt(kw.pop("img", img), **kw)
            except AdapterError as ex:
                ok = str(ex).startswith("-2:") and text in str(ex) and (ad.pts == STALE).all()
                return ok, "%s; outputs untouched: %s" % (ex, (ad.pts == STALE).all())
            return False, "accepted: %d corners" % got[1]
        return run

    rep.guarded("corners beyond the capacity: refused, the text names the capacity", refused("capacity", img=flood, max_corners=0, min_distance=0.0))
    rep.guarded("corners after the refusal", lambda: same_corners(ad.gftt(img, mask), want_mask))
    rep.guarded("refusal: a mask of another size", refused("mask", mask=np.ascontiguousarray(mask[:, :130])))
    rep.guarded("refusal: a mask of another height", refused("mask", mask=np.ascontiguousarray(mask[:66])))
    rep.guarded("refusal: a mask that is not CV_8UC1", refused("mask", mask=np.zeros((67, 131 * 4), np.uint8), mask_type=CV_32FC1, mask_shape=(67, 131)))
    rep.guarded("refusal: an image that is not 8-bit", refused("8-bit", img=np.zeros((67, 131 * 4), np.uint8), img_type=CV_32FC1))
    rep.guarded("corners after the refusals", lambda: same_corners(ad.gftt(img), want_plain))

    # ---- the kept pair across the other entry points ----
    w_A = want_cm("full01", L[0], R[0], L[1], R[1], pts596)
    w_B = want_cm("full12", L[1], R[1], L[2], R[2], w_A["l1"])
    rep.check("premise state: both matchings keep and lose points", 100 < w_A["n_out"] < 596 and 50 < w_B["n_out"] < w_A["n_out"], (w_A["n_out"], w_B["n_out"]))
    ad.keep_pair(True)
    for between, grows in (("featureDetectionGoodFeaturesToTrack_hip", 1), ("featureTracking_hip", 0)):
        k0 = ad.kept_calls()
        rep.guarded("state, %s between: matching A" % between, lambda: same_matching(ad.circular_matching(L[0], R[0], L[1], R[1], pts596), w_A))
        if grows:
            rep.guarded("state: the detection between A and B", lambda: same_corners(ad.gftt_default(L[1]), ref_gftt(L[1])))
        else:
            rep.guarded("state: the tracking between A and B", lambda: same_tracking(ad.feature_tracking(L[0], R[0], pts596), orc.ref_feature_tracking(L[0], R[0], pts596)))
        rep.guarded("state, %s between: matching B on A's t1 buffers" % between, lambda: same_matching(ad.circular_matching(L[1], R[1], L[2], R[2], w_A["l1"]), w_B))
        rep.check("state, %s between: kept calls grow by %d" % (between, grows), ad.kept_calls() - k0 == grows, ad.kept_calls() - k0)
    ad.keep_pair(False)

    print(json.dumps({"checks": rep.checks, "details": rep.details, "inputs": crc(seq)}))
    return 0 if all(rep.checks.values()) else 1


if __name__ == "__main__":
    try:
        rc = main()
    except BaseException:   # noqa: BLE001  (1 means "a check is false" and comes with the JSON line; anything else is a death)
        import traceback
        traceback.print_exc()
        rc = 3
    sys.exit(rc)
