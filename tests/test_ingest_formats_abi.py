"""Input formats (vo_params.input_format, VO_FMT_*) at the interface, without a device: the header declares the constants and
the field, the ctypes mirror has the C struct's size, the defaults are gray, and the image helpers of visual_odom_amd/_lib.py
turn colour arrays and the planes of an interleaved frame into the right pointer / byte stride -- or refuse them."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

from visual_odom_amd import _lib

HEADER = os.path.join(ROOT, "include", "vo_hip.h")
FORMATS = dict(VO_FMT_GRAY8=0, VO_FMT_GRAY8_X2=1, VO_FMT_BGR8=2, VO_FMT_RGB8=3, VO_FMT_BGRA8=4, VO_FMT_RGBA8=5)


def test_header_declares_the_formats_and_the_field():
    text = open(HEADER).read()
    for name, value in FORMATS.items():
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), text), name
        assert getattr(_lib, name.replace("VO_", "")) == value
    body = re.search(r"typedef struct vo_params \{(.*?)\} vo_params;", text, re.S).group(1)
    fields = re.findall(r"^\s*(?:int|float|double)\s+(\w+);", body, re.M)
    assert fields[-1] == "input_format", "the new field goes at the END of vo_params"
    assert fields == [n for n, _ in _lib.VoParams._fields_], "ctypes mirror and header list the same fields in the same order"
    assert _lib.FMT_BPP == (1, 2, 3, 3, 4, 4)


def test_ctypes_struct_has_the_size_of_the_c_struct(tmp_path):
    src = tmp_path / "sizeof_params.c"
    src.write_text('#include <stdio.h>\n#include "vo_hip.h"\n'
                   'int main(void) { printf("%zu %zu\\n", sizeof(vo_params), offsetof(vo_params, input_format)); return 0; }\n')
    exe = str(tmp_path / "sizeof_params")
    subprocess.check_call(["gcc", "-include", "stddef.h", "-I" + os.path.join(ROOT, "include"), "-o", exe, str(src)])
    size, off = (int(v) for v in subprocess.check_output([exe], text=True).split())
    assert C.sizeof(_lib.VoParams) == size
    assert _lib.VoParams.input_format.offset == off


def test_default_params_are_gray():
    lib = _lib.load()   # (the library loads without a device; only vo_create needs one)
    p = _lib.VoParams()
    p.input_format = 77
    lib.vo_default_params(C.byref(p))
    assert p.input_format == _lib.FMT_GRAY8 and p.lk_max_level == 3


def test_the_feature_adds_no_entry_point():
    assert not any("fmt" in s or "format" in s or "ingest" in s for s in _lib.EXPORTS)


@pytest.mark.parametrize("fmt,bpp", [(_lib.FMT_BGR8, 3), (_lib.FMT_RGB8, 3), (_lib.FMT_BGRA8, 4), (_lib.FMT_RGBA8, 4)])
def test_colour_arrays_pointer_and_stride(fmt, bpp):
    h, w = 12, 40
    a, b = np.zeros((h, w, bpp), np.uint8), np.ones((h, w, bpp), np.uint8)
    arrs, stride = _lib._imgs(a, b, fmt=fmt)
    assert stride == w * bpp and arrs[0].ctypes.data == a.ctypes.data and arrs[1].ctypes.data == b.ctypes.data   # as they are
    # a padded buffer / an ROI of a bigger image: passed as it is, with its stride
    big = np.zeros((h + 3, w + 9, bpp), np.uint8)
    roi = big[2:2 + h, 5:5 + w]
    (r,), stride = _lib._imgs(roi, fmt=fmt)
    assert stride == (w + 9) * bpp and r.ctypes.data == big.ctypes.data + 2 * stride + 5 * bpp
    # not pixel-contiguous (a channel-reversed view): copied, never misread
    (c,), stride = _lib._imgs(a[..., ::-1], fmt=fmt)
    assert stride == w * bpp and c.flags.c_contiguous
    # None stays None
    arrs, stride = _lib._imgs_opt(None, None, a, b, fmt=fmt)
    assert arrs[0] is None and arrs[1] is None and arrs[2].shape == (h, w, bpp) and stride == w * bpp
    for bad in (np.zeros((h, w), np.uint8), np.zeros((h, w, 7 - bpp), np.uint8), np.zeros((h, w, bpp), np.uint16)):
        with pytest.raises(ValueError):
            _lib._imgs(bad, fmt=fmt)
    with pytest.raises(ValueError):
        _lib._imgs(a, np.zeros((h, w + 1, bpp), np.uint8), fmt=fmt)


def test_interleaved_planes_pointer_and_stride():
    h, w = 10, 36
    buf = np.arange(h * w, dtype=np.uint16)                 # the sensor's frame: one 16-bit word per pixel pair
    planes = buf.view(np.uint8).reshape(h, w, 2)
    left, right = planes[..., 0], planes[..., 1]
    arrs, stride = _lib._imgs(left, right, fmt=_lib.FMT_GRAY8_X2)
    assert stride == 2 * w
    assert arrs[0].ctypes.data == buf.ctypes.data and arrs[1].ctypes.data == buf.ctypes.data + 1   # left = buf, right = buf + 1
    # what the foreign call receives is the view's first byte
    assert C.cast(_lib._p(arrs[1]), C.c_void_p).value == buf.ctypes.data + 1
    # a padded frame
    pad = np.zeros((h, 2 * w + 6), np.uint8)
    v = np.lib.stride_tricks.as_strided(pad, (h, w, 2), (2 * w + 6, 2, 1))
    arrs, stride = _lib._imgs(v[..., 0], v[..., 1], fmt=_lib.FMT_GRAY8_X2)
    assert stride == 2 * w + 6 and arrs[1].ctypes.data == pad.ctypes.data + 1
    # a plain gray image, a colour image, planes of different pitch: refused before any C call
    for bad in (np.zeros((h, w), np.uint8), np.zeros((h, w, 3), np.uint8), buf.reshape(h, w)):
        with pytest.raises(ValueError):
            _lib._imgs(bad, fmt=_lib.FMT_GRAY8_X2)
    with pytest.raises(ValueError):
        _lib._imgs(left, v[..., 1], fmt=_lib.FMT_GRAY8_X2)


def test_gray_helper_is_what_it_was_and_unknown_formats_raise():
    a = np.zeros((8, 40), np.uint8)
    (g,), stride = _lib._imgs(a)
    assert stride == 40 and g.ctypes.data == a.ctypes.data
    (g,), stride = _lib._imgs(a[:, ::2])   # gray: anything else is made contiguous, as before
    assert stride == 20 and g.flags.c_contiguous
    for fmt in (6, -1):
        with pytest.raises(ValueError):
            _lib._imgs(a, fmt=fmt)


def test_context_helpers_use_the_context_format_without_a_device():
    """the host logic alone: a Context object whose vo_ctx is never created (no device), set to a colour format"""
    ctx = _lib.Context.__new__(_lib.Context)
    ctx.h = None
    ctx.input_format = _lib.FMT_BGR8
    seen = {}

    class Lib:
        def vo_batch_upload_image(self, h, idx, ptr, stride):
            seen["stride"] = stride
            return 0
    ctx.lib = Lib()
    ctx.batch_upload_image(0, np.zeros((6, 34, 3), np.uint8))
    assert seen["stride"] == 34 * 3
    with pytest.raises(ValueError):
        ctx.batch_upload_image(0, np.zeros((6, 34), np.uint8))   # a gray image does not fit a BGR context


def test_run_cli_keeps_rgb_files_as_rgb_for_the_device(tmp_path):
    """visual_odom_amd.run --device-convert: the decoded file as (h, w, 3) RGB, gray files replicated; the default path still
    folds to gray on the host"""
    from PIL import Image
    from visual_odom_amd import run
    rng = np.random.default_rng(3)
    rgb = rng.integers(0, 256, (9, 33, 3), dtype=np.uint8)
    gray = rng.integers(0, 256, (9, 33), dtype=np.uint8)
    for cam, img in ((0, rgb), (1, gray)):
        d = tmp_path / ("image_%d" % cam)
        d.mkdir()
        Image.fromarray(img).save(str(d / "000000.png"))
    left, right = run.read_pair(str(tmp_path), 0, rgb=True)
    assert np.array_equal(left, rgb) and np.array_equal(right, np.repeat(gray[..., None], 3, axis=2))
    arrs, stride = _lib._imgs(left, right, fmt=_lib.FMT_RGB8)
    assert stride == 33 * 3
    left, right = run.read_pair(str(tmp_path), 0)
    p = rgb.astype(np.int64)
    assert np.array_equal(left, ((p[..., 2] * 1868 + p[..., 1] * 9617 + p[..., 0] * 4899 + 8192) >> 14).astype(np.uint8))
    assert np.array_equal(right, gray) and run.read_pair(str(tmp_path), 1, rgb=True) is None
