"""The converting ingest kernels (visual_odom_amd/csrc/ingest_fmt.hip: seq_ingest_fmt_kernel, pull_image_fmt_kernel) executed on
the CPU through the coroutine SIMT emulator (tests/host_check/hip_emu.h + ingest_fmt_emu.cpp) and compared BIT FOR BIT with a
few lines of numpy: the integer colour formula of include/vo_hip.h and plane slicing for the two-byte interleave.

Every source image sits in a heap block of its own of exactly the bytes the format's contract lets a kernel read (the harness
copies it there), so under VO_SANITIZE=1 (LD_PRELOAD=libasan.so, the way tests/test_sanitize.py starts its child) an over-read
is an AddressSanitizer abort.  Every destination row is checked OUTSIDE its w columns too (guard pattern).  The lock-step
kernel runs with fewer and with more waves than rows; the pull kernel's grid is a function of the shape (its launcher's), so it
has one grid per case, plus the workgroups that carry the call's points.  Unit test of device code, not a product path."""
import ctypes as C

import numpy as np
import pytest

import emu_build
from conftest import BUILD_DIR, SAN_FLAGS, vp

GRAY8_X2, BGR8, RGB8, BGRA8, RGBA8 = 1, 2, 3, 4, 5
BPP = {GRAY8_X2: 2, BGR8: 3, RGB8: 3, BGRA8: 4, RGBA8: 4}
NAMES = {GRAY8_X2: "gray8_x2", BGR8: "bgr8", RGB8: "rgb8", BGRA8: "bgra8", RGBA8: "rgba8"}
WIDTHS = [32, 33, 39, 64, 519, 640, 1241]
GUARD = 0xA5


@pytest.fixture(scope="module")
def ife():
    lib = emu_build.shared("ingest_fmt_emu", SAN_FLAGS, BUILD_DIR)
    lib.ife_seq_ingest.restype = C.c_int
    lib.ife_pull.restype = C.c_int
    return lib


def to_gray(px, fmt):
    """numpy's answer: px (h, w, bpp) uint8 -> (h, w) uint8"""
    p = px.astype(np.int64)
    if fmt == GRAY8_X2:
        return px[..., 0].copy()
    b, g, r = (p[..., 0], p[..., 1], p[..., 2]) if fmt in (BGR8, BGRA8) else (p[..., 2], p[..., 1], p[..., 0])
    return ((b * 1868 + g * 9617 + r * 4899 + 8192) >> 14).astype(np.uint8)


def raw_image(rng, fmt, w, h, stride):
    """(pixels (h, w, bpp), the exact bytes a kernel may read: (h - 1) * stride + row bytes, padding filled with noise)"""
    bpp = BPP[fmt]
    px = rng.integers(0, 256, (h, w, bpp), dtype=np.uint8)
    px[0, :8] = 255   # the formula's extremes
    px[0, 8:16] = 0
    row_bytes = 2 * w - 1 if fmt == GRAY8_X2 else w * bpp
    buf = rng.integers(0, 256, (h - 1) * stride + row_bytes, dtype=np.uint8)
    for y in range(h):
        buf[y * stride:y * stride + row_bytes] = px[y].reshape(-1)[:row_bytes]
    return px, buf


def check_dst(dst, want, w):
    """dst (n, h, pitch): columns [0, w) == want, everything else still the guard"""
    assert np.array_equal(dst[:, :, :w], want)
    assert np.all(dst[:, :, w:] == GUARD), "a destination byte outside the w columns of a row changed"


def ptr_array(bufs):
    return (C.c_void_p * len(bufs))(*[b.ctypes.data for b in bufs])


@pytest.mark.parametrize("padded", [False, True], ids=["tight", "padded"])
@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("fmt", sorted(BPP), ids=lambda f: NAMES[f])
def test_seq_ingest_fmt_kernel(ife, fmt, w, padded):
    h, n_pairs = 5, 2
    stride = w * BPP[fmt] + (13 if padded else 0)
    pitch = (32 + w + 24 + 15) // 16 * 16
    rng = np.random.default_rng(1000 * fmt + w + padded)
    imgs = [raw_image(rng, fmt, w, h, stride) for _ in range(2 * n_pairs)]
    want = np.stack([to_gray(px, fmt) for px, _ in imgs])
    left, right = [b for _, b in imgs[0::2]], [b for _, b in imgs[1::2]]
    for n_waves in (3, 2 * n_pairs * h + 11):   # fewer and more waves than rows
        dst = np.full((2 * n_pairs, h, pitch), GUARD, np.uint8)
        rc = ife.ife_seq_ingest(fmt, ptr_array(left), ptr_array(right), C.c_size_t(left[0].size), n_pairs, w, h, stride, pitch, vp(dst),
                                n_waves)
        assert rc == 0
        check_dst(dst, want, w)


@pytest.mark.parametrize("padded", [False, True], ids=["tight", "padded"])
@pytest.mark.parametrize("w", WIDTHS)
def test_seq_ingest_interleaved_pair_read_once(ife, w, padded):
    """Y8I: ONE buffer of 16-bit words per pair, left = buf, right = buf + 1 -- the kernel's read-once path; the buffer ends with
    the last word of the last row"""
    h, n_pairs = 5, 2
    stride = 2 * w + (14 if padded else 0)
    pitch = (32 + w + 24 + 15) // 16 * 16
    rng = np.random.default_rng(77 + w + padded)
    bufs, want = [], []
    for _ in range(n_pairs):
        buf = rng.integers(0, 256, (h - 1) * stride + 2 * w, dtype=np.uint8)
        rows = np.stack([buf[y * stride:y * stride + 2 * w] for y in range(h)]).reshape(h, w, 2)
        bufs.append(buf)
        want += [rows[..., 0], rows[..., 1]]
    want = np.stack(want)
    for n_waves in (3, 2 * n_pairs * h + 11):
        dst = np.full((2 * n_pairs, h, pitch), GUARD, np.uint8)
        rc = ife.ife_seq_ingest(GRAY8_X2, ptr_array(bufs), None, C.c_size_t(bufs[0].size), n_pairs, w, h, stride, pitch, vp(dst), n_waves)
        assert rc == 0
        check_dst(dst, want, w)


def test_seq_ingest_two_planes_of_one_buffer_as_independent_images(ife):
    """the right plane handed over on its own (a pair whose left is elsewhere): rows are read up to their last pixel only, which
    is what keeps `buf + 1` inside the frame"""
    w, h = 39, 4
    stride, pitch = 2 * w, 96
    rng = np.random.default_rng(5)
    frame = rng.integers(0, 256, (h, w, 2), dtype=np.uint8)
    other = rng.integers(0, 256, (h, w, 2), dtype=np.uint8)
    right_plane = frame.reshape(-1)[1:]           # 2 w h - 1 bytes: starts at byte 1, ends with the frame
    left_plane = other.reshape(-1)[:-1].copy()    # (an independent buffer of the same length)
    right_plane = right_plane.copy()
    dst = np.full((2, h, pitch), GUARD, np.uint8)
    rc = ife.ife_seq_ingest(GRAY8_X2, ptr_array([left_plane]), ptr_array([right_plane]), C.c_size_t(right_plane.size), 1, w, h, stride,
                            pitch, vp(dst), 7)
    assert rc == 0
    check_dst(dst, np.stack([other[..., 0], frame[..., 1]]), w)


@pytest.mark.parametrize("padded", [False, True], ids=["tight", "padded"])
@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("fmt", sorted(BPP), ids=lambda f: NAMES[f])
def test_pull_image_fmt_kernel(ife, fmt, w, padded):
    h = 6
    stride = w * BPP[fmt] + (13 if padded else 0)
    pitch = (32 + w + 24 + 15) // 16 * 16
    rng = np.random.default_rng(2000 * fmt + w + padded)
    px, buf = raw_image(rng, fmt, w, h, stride)
    n_pts = 300 if w == 640 else 0   # (one width also carries the call's points and their count, like the last image of a call)
    pts = rng.random((max(n_pts, 1), 2), dtype=np.float32)
    pts_dst = np.zeros_like(pts)
    count = C.c_int(-1)
    dst = np.full((1, h, pitch), GUARD, np.uint8)
    rc = ife.ife_pull(fmt, vp(buf), C.c_size_t(buf.size), stride, vp(dst), pitch, w, h, vp(pts), vp(pts_dst) if n_pts else None, n_pts,
                      C.byref(count) if n_pts else None)
    assert rc == 0
    check_dst(dst, to_gray(px, fmt)[None], w)
    if n_pts:
        assert count.value == n_pts and np.array_equal(pts_dst, pts)


def test_unknown_format_has_no_kernel(ife):
    buf = np.zeros(64 * 4, np.uint8)
    dst = np.full((1, 1, 128), GUARD, np.uint8)
    for fmt in (0, 6, -1):   # (gray never reaches this file: the gray kernels move it)
        assert ife.ife_pull(fmt, vp(buf), C.c_size_t(buf.size), 256, vp(dst), 128, 32, 1, None, None, 0, None) == -1
    assert np.all(dst == GUARD)
