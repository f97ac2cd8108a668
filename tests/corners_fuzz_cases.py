"""The seeded fuzz of the Shi-Tomasi detector: the generator and its checks, with the side under test behind a small backend, so that
the SAME cases run through the device (test_gpu_corners_fuzz.py), through the coroutine emulator (test_corners_scale_emulation.py: a
mismatch there is a logic error, one on the device alone points at the concurrent parts of corn_select_kernel) and through nothing
at all (backend None: the reference alone must meet the floors of check_floors).

A case is a region of interest -- a view with stride 640 -- of one of seven 640 x 256 sources, with a min_distance, a quality_level
and a max_corners from lists that reach the kernel's edges: widths on both sides of corn_map_kernel's seams, distances around the
`lim <= 1` shortcut and the half-to-even cell sizes, lists beyond 1024 and 2048 candidates and beyond the capacity.  Expected values
are corners_emu.ref_detect (tests/host_check/corners_ref.c) and, under a mask, corners_mask_cases.ref_detect; everything is identity.

Conventions of test_detect_bucket_fuzz: VO_FUZZ_EXAMPLES, VO_FUZZ_SEED (derandomized unless a seed is given), no example database,
a `seen` dictionary that the caller prints.  hypothesis mixes the constants of the modules a session has imported into its draws, so
the cases of a derandomized run are the same from run to run of one command, not from one selection of test modules to another:
the floors are held with room to spare (300 cases, eight sessions and seeds: 2 .. 16 refused, 69 .. 96 under a mask)."""
import os

import numpy as np

import corners_emu as ce
import corners_mask_cases as cm
import corners_scale as cs

SRC_W, SRC_H = 640, 256
WIDTHS = [32, 33, 64, 97, 131, 200, 254, 255, 256, 300, 333, 480, 509, 601, 640]
HEIGHTS = [32, 33, 40, 64, 97, 128, 160, 200, 256]
DISTANCES = [0.0] + cs.DISTANCES + [2.0, 3.0, 4.9, 5.0, 7.5, 10.5, 17.3, 32.0]
QUALITIES = [1e-6, 1e-3, 0.01, 0.01, 0.01, 0.05, 0.3, 1.0]
MAX_CORNERS = [0, 0, 0, 1, 17, 500, 5000]
MASKS = [("left_half", lambda w, h, seed: cm.left_half(w, h)), ("checker", lambda w, h, seed: cm.checker(w, h)),
         ("random_half", cm.random_half), ("all_zero", lambda w, h, seed: np.zeros((h, w), np.uint8))]
MASKED_BELOW = 3000   # candidates of the masked reference up to which a case runs under its mask (that reference's suppression is a python loop)
MAX_KEPT = 60         # kept points of a replenish case (a context takes up to its max_pts)


def sources():
    yy, xx = np.mgrid[0:SRC_H, 0:SRC_W]
    board = (((xx // 5 + yy // 5) & 1) * 200 + 20).astype(np.uint8)
    return [ce.noise(SRC_W, SRC_H, 5), board, ce.blobs(SRC_W, SRC_H, 6, count=400), ce.periodic(SRC_W, SRC_H, 4), cs.tiles(SRC_W, SRC_H, cols=200),
            ce.dark_highlights(SRC_W, SRC_H, 7), ce.squares(SRC_W, SRC_H, 8)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class EmuBackend:
    """the product's kernels through the coroutine emulator, with the capacity of the fuzz's device context"""
    capacity = cs.CAPACITY

    def map(self, img):
        return ce.emu_map(np.ascontiguousarray(img), stride=img.strides[0])

    def detect(self, img, mask, mc, q, md):
        """(corners, n), or None for a refused run"""
        if mask is None:
            pts, n = ce.emu_detect([np.ascontiguousarray(img)], mc, q, md, cap=self.capacity, lcap=self.capacity, stride=img.strides[0])[0][:2]
        else:
            pts, n = cm.emu_detect([np.ascontiguousarray(img)], [mask], mc, q, md, cap=self.capacity, lcap=self.capacity, stride=img.strides[0],
                                   mask_stride=img.shape[1] + 9)[0][:2]
        return None if n < 0 else (pts, n)

    def replenish(self, img, kept, radius, mc, q, md):
        h, w = img.shape
        return self.detect(img, cm.emu_disc(w, h, kept, radius, mask_stride=w + 3), mc, q, md)


class DeviceBackend:
    """vocorn_min_eigen_map, vocorn_detect, vocmask_detect and vocmask_replenish of a context, called with their outputs full of a
    stale value: a refused run (VO_ERR_OVERFLOW) must leave n_out and the buffer as they were, an accepted one every row beyond
    its corners.  ctx: a visual_odom_amd._lib.Context; volib: that module"""
    STALE = -5.0

    def __init__(self, ctx, volib, max_w, max_h):
        self.ctx, self.volib = ctx, volib
        self.capacity = max(4 * ctx.max_pts, 16384, max_w * max_h // 16)   # include/vo_hip.h: the corner-list capacity of vo_create(max_w, max_h, max_pts)
        self.rows = self.capacity + 8

    def map(self, img):
        return self.ctx.corner_min_eigen_val(img)

    @staticmethod
    def _view(a):
        assert a.dtype == np.uint8 and a.ndim == 2 and a.strides[1] == 1 and a.strides[0] >= a.shape[1]
        return a.ctypes.data, int(a.strides[0])

    def _call(self, fn):
        import ctypes as C
        pts = np.full((self.rows, 2), self.STALE, np.float32)
        n = C.c_int(-77)
        rc = fn(pts.ctypes.data, self.rows, C.byref(n))
        if rc == self.volib.VO_ERR_OVERFLOW:
            assert n.value == -77 and (pts == self.STALE).all(), "a refused run wrote to its outputs"
            assert b"capacity" in self.ctx.lib.vo_last_error(self.ctx.h)
            return None
        assert rc == 0, (rc, self.ctx.lib.vo_last_error(self.ctx.h))
        assert 0 <= n.value <= self.capacity and (pts[n.value:] == self.STALE).all(), "rows beyond the corners were written"
        return pts[:n.value].copy(), n.value

    def detect(self, img, mask, mc, q, md):
        """(corners, n), or None for a refused run.  img (and mask): views, passed with their own strides"""
        import ctypes as C
        lib, h = self.ctx.lib, self.ctx.h
        prm = self.volib.VoCornParams(int(mc), float(q), float(md))
        ip, stride = self._view(img)
        ih, iw = img.shape
        if mask is None:
            return self._call(lambda pts, cap, n: lib.vocorn_detect(h, ip, iw, ih, stride, C.byref(prm), pts, cap, n))
        mview = ce.strided(mask, iw + 9)[:, :iw]                          # a byte stride that is not the width
        mp, ms = self._view(mview)
        return self._call(lambda pts, cap, n: lib.vocmask_detect(h, ip, iw, ih, stride, mp, ms, C.byref(prm), pts, cap, n))

    def replenish(self, img, kept, radius, mc, q, md):
        import ctypes as C
        lib, h = self.ctx.lib, self.ctx.h
        prm = self.volib.VoCornParams(int(mc), float(q), float(md))
        ip, stride = self._view(img)
        ih, iw = img.shape
        k = np.ascontiguousarray(kept, np.float32).reshape(-1, 2)
        kp = k.ctypes.data if len(k) else None
        return self._call(lambda pts, cap, n: lib.vocmask_replenish(h, ip, iw, ih, stride, kp, len(k), int(radius), C.byref(prm), pts, cap, n))


def kept_points(rng, w, h):
    """0 .. MAX_KEPT points: inside, on half pixels (2.5 -> 2, 3.5 -> 4), a little outside"""
    n = int(rng.integers(0, MAX_KEPT + 1))
    k = np.stack([rng.uniform(-6, w + 6, n), rng.uniform(-6, h + 6, n)], 1)
    half = rng.random(n) < 0.3
    k[half] = np.floor(k[half]) + 0.5
    return k.astype(np.float32)


def run(backend, n_examples=None, explore=None, default_examples=300):
    """the fuzz over `backend` (None: the reference alone).  Returns the `seen` dictionary"""
    from hypothesis import HealthCheck, given, settings, strategies as st
    n_examples = int(os.environ.get("VO_FUZZ_EXAMPLES", str(default_examples))) if n_examples is None else n_examples
    srcs = sources()
    capacity = cs.CAPACITY if backend is None else backend.capacity
    seen = dict(examples=0, cases=0, over=0, empty=0, long=0, wide=0, maps=0, masked=0, replenished=0, corners=0)

    @settings(max_examples=n_examples, derandomize=explore is None, deadline=None, database=None, suppress_health_check=list(HealthCheck))
    @given(seed=st.integers(0, 2 ** 31 - 1), src=st.integers(0, 6), w=st.sampled_from(WIDTHS), h=st.sampled_from(HEIGHTS),
           md=st.sampled_from(DISTANCES), q=st.sampled_from(QUALITIES), mc=st.sampled_from(MAX_CORNERS))
    def case(seed, src, w, h, md, q, mc):
        seen["examples"] += 1
        rng = np.random.default_rng([seed, src, w, h, int(md * 100), int(q * 1e6), mc])
        k = int(rng.integers(0, 105))                                   # every fifth, third, seventh case -- by the case's own draw, not by
                                                                        # its place in the run, so that a case replays as it ran
        x0, y0 = int(rng.integers(0, SRC_W - w + 1)), int(rng.integers(0, SRC_H - h + 1))
        if src == 4:
            x0 = min(x0, 60)                                            # (tiles: at least 140 of the pattern's 200 columns, and their right
                                                                        # edge; a third of these regions hold more candidates than the capacity)
        img = srcs[src][y0:y0 + h, x0:x0 + w]                           # a view: stride 640
        cont = np.ascontiguousarray(img)
        what = (seed, src, w, h, md, q, mc)
        if k % 5 == 0:
            seen["maps"] += 1
            if backend is not None:
                assert np.array_equal(bits(backend.map(img)), bits(ce.ref_map(cont))), ("map",) + what
        want, n, ncand = ce.ref_detect(cont, mc, q, md)
        seen["wide"] += w > 254
        seen["long"] += ncand > 2048
        if ncand > capacity:                                            # refused, nothing written (the backend checks that): never skipped
            seen["over"] += 1
            if backend is not None:
                assert backend.detect(img, None, mc, q, md) is None, ("accepted beyond the capacity", ncand) + what
            return
        seen["cases"] += 1
        seen["empty"] += n == 0
        seen["corners"] += n
        if backend is not None:
            got = backend.detect(img, None, mc, q, md)
            assert got is not None and got[1] == n and np.array_equal(bits(got[0]), bits(want)), ("corners", None if got is None else got[1], n, ncand) + what
        if k % 3 == 0:
            mname, gen = MASKS[int(rng.integers(0, len(MASKS)))]
            mask = gen(w, h, int(rng.integers(0, 1000)))
            if cm.ref_detect(cont, mask, 1, q, 0.0)[2] <= MASKED_BELOW:         # (its candidate count alone: the loop stops at one corner)
                mwant, mn, _ = cm.ref_detect(cont, mask, mc, q, md)
                seen["masked"] += 1
                if backend is not None:
                    got = backend.detect(img, mask, mc, q, md)
                    assert got is not None and got[1] == mn and np.array_equal(bits(got[0]), bits(mwant)), ("mask " + mname, got[1], mn) + what
        if k % 7 == 0:
            kept, radius = kept_points(rng, w, h), int(rng.choice([0, 1, 3, 5, 12, 40]))
            disc = cm.ref_disc_mask(w, h, kept, radius)
            if cm.ref_detect(cont, disc, 1, q, 0.0)[2] <= MASKED_BELOW:
                rwant, rn, _ = cm.ref_detect(cont, disc, mc, q, md)
                seen["replenished"] += 1
                if backend is not None:
                    got = backend.replenish(img, kept, radius, mc, q, md)
                    assert got is not None and got[1] == rn and np.array_equal(bits(got[0]), bits(rwant)), ("replenish", len(kept), radius, got[1], rn) + what

    if explore is not None:
        from hypothesis import seed as hyp_seed
        case = hyp_seed(int(explore))(case)
    case()
    return seen


def check_floors(seen):
    """what a run must have reached to count as one (the value lists above are tuned to these, never the other way round)"""
    e = seen["examples"]
    assert seen["cases"] >= 0.8 * e, seen
    assert 0 < seen["over"] <= 0.1 * e, seen
    assert seen["empty"] <= 0.25 * e, seen
    assert seen["long"] >= 0.05 * e, seen
    assert seen["wide"] >= 0.3 * e, seen
    assert seen["masked"] >= 0.2 * e, seen
