"""The Shi-Tomasi detector under a mask (include/vo_corners_mask.h) as the tests see it: the reference, the case table, and the
product's masked kernels run through the coroutine emulator (tests/host_check/corners_emu.cpp).

THE REFERENCE is independent of the kernels.  The quality map is corners_ref.c's (corners_emu.ref_map); the rest is what OpenCV 4.5's
goodFeaturesToTrack does with a mask, in numpy: minMaxLoc over the allowed pixels (f64; 0 when there is none), threshold(TOZERO) at
(float)(max * qualityLevel) and the 3 x 3 dilate on the UNMASKED map, the candidate test `val != 0 && val == dilated && mask != 0`
on the interior, the sort by (quality descending, address descending) and upstream's grid loop (cell cvRound(minDistance), conflict
iff dx^2 + dy^2 < minDistance^2, stop at maxCorners).  Without a mask it is corners_ref.c's cr_detect (test_corners_mask_emulation.py
checks that first).  THE DISC MASK reference is written from the header's definition.

The libraries loaded into python are built WITHOUT sanitizer flags whatever the environment says.  The sanitizer tier is the same
harness as a STAND-ALONE program with its own main(), built with -fsanitize=address,undefined (runtimes linked statically) and run
as a child, as corners_emu.run_standalone does.  Nothing instrumented is loaded into python."""
import numpy as np

import corners_emu as ce
import emu_build
from conftest import vp


# ---- the reference -----------------------------------------------------------------------------------------------------------

def ref_detect(img, mask=None, max_corners=0, quality_level=0.01, min_distance=5.0):
    """(corners [n, 2] float32, n, candidates) of cv::goodFeaturesToTrack(img, ..., mask, 3, false, 0.04)"""
    eig = ce.ref_map(img)
    h, w = eig.shape
    allowed = np.ones((h, w), bool) if mask is None else (np.asarray(mask) != 0)
    assert allowed.shape == (h, w)
    max_val = float(eig[allowed].max()) if allowed.any() else 0.0                 # minMaxLoc(eig, 0, &maxVal, 0, 0, mask): a double
    thresh = np.float32(max_val * float(quality_level))
    val = np.where(eig > thresh, eig, np.float32(0))                              # threshold(TOZERO), on the whole map
    pad = np.full((h + 2, w + 2), -np.inf, np.float32)
    pad[1:-1, 1:-1] = val
    dil = np.max([pad[j:j + h, k:k + w] for j in range(3) for k in range(3)], axis=0)   # dilate 3 x 3, on the whole map
    cand = (val != 0) & (val == dil) & allowed
    cand[0, :] = cand[-1, :] = False
    cand[:, 0] = cand[:, -1] = False
    ys, xs = np.nonzero(cand)
    q = val[ys, xs]
    order = np.lexsort((-(ys * w + xs), -q.astype(np.float64)))                   # greaterThanPtr: quality, then address, descending
    out = []
    if min_distance >= 1:
        cell = int(np.rint(min_distance))                                         # cvRound
        gw, gh = (w + cell - 1) // cell, (h + cell - 1) // cell
        grid = [[] for _ in range(gw * gh)]
        md2 = float(min_distance) * float(min_distance)
        for i in order:
            x, y = int(xs[i]), int(ys[i])
            xc, yc = x // cell, y // cell
            good = True
            for yy in range(max(yc - 1, 0), min(yc + 1, gh - 1) + 1):
                for xx in range(max(xc - 1, 0), min(xc + 1, gw - 1) + 1):
                    for px, py in grid[yy * gw + xx]:
                        if (x - px) * (x - px) + (y - py) * (y - py) < md2:
                            good = False
                            break
                    if not good:
                        break
                if not good:
                    break
            if good:
                grid[yc * gw + xc].append((x, y))
                out.append((x, y))
                if max_corners > 0 and len(out) == max_corners:
                    break
    else:
        for i in order:
            out.append((int(xs[i]), int(ys[i])))
            if max_corners > 0 and len(out) == max_corners:
                break
    return np.array(out, np.float32).reshape(-1, 2), len(out), int(len(ys))


def ref_disc_mask(w, h, kept, radius):
    """the disc mask of include/vo_corners_mask.h: (h, w) uint8"""
    m = np.full((h, w), 255, np.uint8)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.int64)
    for x, y in np.asarray(kept, np.float32).reshape(-1, 2):
        if not (np.isfinite(x) and np.isfinite(y)) or abs(float(x)) >= 2.0 ** 30 or abs(float(y)) >= 2.0 ** 30:
            continue
        cx, cy = int(np.rint(x)), int(np.rint(y))                                # round half to even, as lrintf
        m[(xx - cx) ** 2 + (yy - cy) ** 2 <= int(radius) * int(radius)] = 0
    return m


# ---- the case table ----------------------------------------------------------------------------------------------------------

def left_half(w, h):
    m = np.zeros((h, w), np.uint8)
    m[:, :w // 2] = 1
    return m


def checker(w, h, step=4):
    yy, xx = np.mgrid[0:h, 0:w]
    return (((yy // step + xx // step) & 1) * 255).astype(np.uint8)


def random_half(w, h, seed=11):
    return ((np.random.default_rng(seed).random((h, w)) < 0.5) * 200).astype(np.uint8)


def border_ring(w, h):
    m = np.full((h, w), 255, np.uint8)
    m[1:-1, 1:-1] = 0
    return m


def strong_outside(w, h):
    """(image, mask): faint interior blobs and one strong 4 x 4 square that the mask excludes.  The threshold comes from the maximum
    over the ALLOWED pixels, so the faint blobs are corners; a threshold from the whole map's maximum leaves none"""
    img = ce.blobs(w, h, 5).astype(np.int32) // 4 + 10
    img[h // 2 - 2:h // 2 + 2, w - 8:w - 4] = 255
    mask = np.full((h, w), 255, np.uint8)
    mask[:, w - 14:] = 0
    return img.astype(np.uint8), mask


STRONG_OUTSIDE_CORNERS = {(32, 32): 1, (65, 33): 3, (131, 67): 22, (300, 40): 28}   # at quality 0.05, min_distance 5
NOISE_MASKS = [("left_half_1", left_half), ("checker_4", checker), ("random_half_200", random_half)]
EMPTY_MASKS = [("all_zero", lambda w, h: np.zeros((h, w), np.uint8)), ("border_ring", border_ring)]
FULL_MASKS = [("all_255", lambda w, h: np.full((h, w), 255, np.uint8)), ("all_1", lambda w, h: np.ones((h, w), np.uint8))]


def mask_cases(w, h):
    """[(name, image, mask, max_corners, quality_level, min_distance)]: the table of the emulator and the GPU tests"""
    out = []
    img = ce.noise(w, h, 21)
    for name, gen in NOISE_MASKS:
        for md in (0.0, 5.0):   # 0: "mask the map before the dilate" differs; 5: "detect unmasked, filter afterwards" differs
            out.append(("noise-%s-md%g" % (name, md), img, gen(w, h), 0, 0.01, md))
    out.append(("noise-checker_4-max17", img, checker(w, h), 17, 0.01, 10.5))
    if w >= 32 and h >= 32:
        simg, smask = strong_outside(w, h)
        out.append(("strong_outside", simg, smask, 0, 0.05, 5.0))
    for name, gen in EMPTY_MASKS + FULL_MASKS:
        out.append(("blobs-" + name, ce.blobs(w, h, 22), gen(w, h), 0, 0.01, 5.0))
    return out


def disc_cases(w, h):
    """[(name, kept [n, 2] float32, radius)]"""
    rng = np.random.default_rng(31)
    sub = np.stack([rng.uniform(0, w, 9), rng.uniform(0, h, 9)], axis=1)
    halves = [(2.5, 3.5), (-0.5, 4.5), (7.5, 0.5), (w - 1.5, h - 0.5)]          # 2.5 -> 2, 3.5 -> 4, -0.5 -> 0
    outside = [(-3.0, h / 2), (w + 2.0, h / 2), (w / 2, -4.0), (w / 2, h + 5.0), (-2.0, -2.0), (w + 1.0, h + 1.0), (-100.0, 5.0)]
    bad = [(np.nan, 5.0), (5.0, np.inf), (-np.inf, 3.0), (1e20, 4.0), (4.0, -1e20), (2.0 ** 30, 3.0), (6.0, 6.0)]
    dup = [(10.2, 9.7), (10.4, 10.1), (9.9, 10.0), (10.0, 10.0)]
    out = []
    for r in (0, 1, 7):
        out += [("subpixel-r%d" % r, sub, r), ("halves-r%d" % r, halves, r), ("outside-r%d" % r, outside, r), ("skipped-r%d" % r, bad, r),
                ("duplicates-r%d" % r, dup, r), ("none-r%d" % r, np.zeros((0, 2)), r)]
    out.append(("whole-image", [(w / 2, h / 2)], 256))
    return [(name, np.asarray(k, np.float32).reshape(-1, 2), r) for name, k, r in out]


# ---- the emulator ------------------------------------------------------------------------------------------------------------

def _pack(imgs, masks, stride, mask_stride):
    h, w = imgs[0].shape
    buf = np.stack([ce.strided(i, stride) for i in imgs])
    on = np.array([m is not None for m in masks], np.uint8)
    mbuf = np.stack([ce.strided(np.zeros((h, w), np.uint8) if m is None else m, mask_stride) for m in masks])
    return buf, mbuf, on


def emu_detect(imgs, masks, max_corners=0, quality_level=0.01, min_distance=5.0, cap=None, lcap=None, stride=None, mask_stride=None, first=0, n=None):
    """images (a list of equal shape) with their masks (None: the image has none) through one emulated run over images first ..
    first + n - 1.  Returns per image of the run (corners, n found or -1 for an overflowed list, candidates)"""
    h, w = imgs[0].shape
    stride = w if stride is None else stride
    mask_stride = w if mask_stride is None else mask_stride
    buf, mbuf, on = _pack(imgs, masks, stride, mask_stride)
    n = len(imgs) - first if n is None else n
    cap = w * h if cap is None else cap
    lcap = w * h if lcap is None else lcap
    pts = np.zeros((n, max(cap, 1), 2), np.float32)
    nout, ncand = np.zeros(n, np.int32), np.zeros(n, np.int32)
    rc = ce.load_emu().cme_detect(vp(buf), vp(mbuf), vp(on), len(imgs), first, n, w, h, stride, mask_stride, max_corners, quality_level, min_distance,
                               lcap, vp(pts), cap, vp(nout), vp(ncand))
    assert rc == 0
    return [(pts[s, :max(0, min(int(nout[s]), cap))].copy(), int(nout[s]), int(ncand[s])) for s in range(n)]


def _unstride(flat, w, h, stride, fill=0xFF):
    """(h, w) out of a block of (h - 1) * stride + w bytes; the bytes between the rows must still hold the fill"""
    full = np.full(h * stride, fill, np.uint8)
    full[:len(flat)] = flat
    full = full.reshape(h, stride)
    assert (full[:, w:] == fill).all(), "a store between the rows of the mask"
    return full[:, :w].copy()


def emu_disc(w, h, kept, radius, mask_stride=None):
    mask_stride = w if mask_stride is None else mask_stride
    k = np.ascontiguousarray(kept, np.float32).reshape(-1, 2)
    out = np.zeros((h - 1) * mask_stride + w, np.uint8)
    assert ce.load_emu().cme_disc(vp(k) if len(k) else None, len(k), int(radius), w, h, mask_stride, vp(out)) == 0
    return _unstride(out, w, h, mask_stride)


def run_standalone(tmp_path, imgs, masks, max_corners, quality_level, min_distance, cap, lcap, kept, radius, stride, mask_stride):
    """the images and masks through the stand-alone ASan + UBSan program, run as a child: no report, exit status 0.  Returns
    ([(corners, n, candidates)], disc mask of `kept`)"""
    exe = emu_build.sanitized_program("corners_emu", "CORNERS_MASK_EMU_MAIN")
    h, w = imgs[0].shape
    n = len(imgs)
    k = np.ascontiguousarray(kept, np.float32).reshape(-1, 2)
    buf, mbuf, on = _pack(imgs, masks, stride, mask_stride)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([n, w, h, stride, mask_stride, max_corners, lcap, cap, len(k), radius], np.int32).tobytes())
        f.write(np.array([quality_level, min_distance], np.float64).tobytes())
        f.write(buf.tobytes() + mbuf.tobytes() + on.tobytes() + k.tobytes())
    emu_build.run_clean(exe, [fin, fout], 600)
    raw = np.fromfile(fout, np.uint8)
    cnt = raw[:8 * n].view(np.int32).reshape(2, n)
    pts = raw[8 * n:8 * n + 8 * n * cap].view(np.float32).reshape(n, cap, 2)
    disc = _unstride(raw[8 * n + 8 * n * cap:], w, h, mask_stride)
    return [(pts[s, :max(0, min(int(cnt[0, s]), cap))].copy(), int(cnt[0, s]), int(cnt[1, s])) for s in range(n)], disc
