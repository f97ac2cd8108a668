"""include/vo_fast_mask.h -- the tenth header, cv::FAST under a mask: it compiles as C99 and as C++11, the ctypes mirror lists exactly
its names (_lib.FAST_MASK_EXPORTS) and lays vofm_params out as the C struct, libvo_hip.so exports exactly them under the vofm prefix
and carries the new kernel, the other prefixes and lists are untouched, and every entry point answers the bad calls that can be decided
without a device with the documented code.  No compute calls."""
import ctypes as C
import os
import re
import subprocess

from test_corners_abi import INC, declared

FM_NAMES = ["vofm_default_params", "vofm_detect", "vofm_get_mask", "vofm_get_params", "vofm_replenish", "vofm_set_params"]
OTHER_PREFIXES = ("vo_", "voflow", "vowin", "voflag", "vocorn", "vocmask", "voresp", "vodet", "votop")
OTHER_HEADERS = ("vo_hip.h", "vo_flow.h", "vo_flow_win.h", "vo_flow_flags.h", "vo_corners.h", "vo_corners_mask.h", "vo_corners_response.h", "vo_detector.h",
                 "vo_topup.h")


def test_fast_mask_header_compiles_as_c_and_cxx11(tmp_path):
    src = tmp_path / "use_fast_mask.c"
    src.write_text('#include <stddef.h>\n#include "vo_fast_mask.h"\n'
                   "typedef char size8[sizeof(vofm_params) == 8 ? 1 : -1];\n"
                   "typedef char off_m[offsetof(vofm_params, mode) == 0 ? 1 : -1];\n"
                   "typedef char off_r[offsetof(vofm_params, radius) == 4 ? 1 : -1];\n"
                   "typedef char top8[sizeof(votop_params) == 8 ? 1 : -1];\n"
                   "typedef char det48[sizeof(vodet_params) == 48 ? 1 : -1];\n"
                   "typedef char modes[VOFM_OFF == 0 && VOFM_CARRIED == 1 ? 1 : -1];\n"
                   "int use(vo_ctx *c, const uint8_t *img, float *pts, int32_t *ages, int *n, uint8_t *mask, const float *kept)\n"
                   "{\n"
                   "    vofm_params p;\n"
                   "    int rc;\n"
                   "    vofm_default_params(&p);\n"
                   "    p.mode = VOFM_CARRIED;\n"
                   "    p.radius = VOCORN_MAX_MIN_DISTANCE;\n"
                   "    rc = vofm_set_params(c, &p) | vofm_get_params(c, &p);\n"
                   "    rc |= vo_detect_bucket(c, img, 64, 48, 64, NULL, pts, n, ages, n, 100);\n"
                   "    rc |= vofm_get_mask(c, 0, mask, 64);\n"
                   "    rc |= vofm_detect(c, img, 64, 48, 64, 20, 1, mask, 64, pts, 100, n);\n"
                   "    rc |= vofm_replenish(c, img, 64, 48, 64, 20, 1, kept, 3, 5, pts, 100, n);\n"
                   "    rc |= vofm_set_params(c, NULL);\n"
                   "    return rc == VO_OK && p.mode != VOFM_OFF ? 0 : VO_ERR_ARG;\n"
                   "}\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I" + INC, str(src)])
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", "-I" + INC, str(src)])


def test_fast_mask_binding_list_matches_header():
    from visual_odom_amd import _lib
    assert declared("vo_fast_mask.h", "vofm_") == FM_NAMES
    assert sorted(_lib.FAST_MASK_EXPORTS) == FM_NAMES
    for prefix in OTHER_PREFIXES:
        assert declared("vo_fast_mask.h", prefix) == [], "nothing under " + prefix
        assert not "vofm".startswith(prefix) and not prefix.startswith("vofm")
    others = (set(_lib.EXPORTS) | set(_lib.FLOW_EXPORTS) | set(_lib.WIN_EXPORTS) | set(_lib.FLAG_EXPORTS) | set(_lib.CORN_EXPORTS) |
              set(_lib.CMASK_EXPORTS) | set(_lib.RESP_EXPORTS) | set(_lib.DET_EXPORTS) | set(_lib.TOPUP_EXPORTS))
    assert not set(_lib.FAST_MASK_EXPORTS) & others
    hdr = open(os.path.join(INC, "vo_fast_mask.h")).read()
    assert '#include "vo_topup.h"' in hdr
    for other in OTHER_HEADERS:
        assert declared(other, "vofm") == [], other + " declares nothing under the new prefix"
    assert (len(_lib.EXPORTS), len(_lib.CORN_EXPORTS), len(_lib.CMASK_EXPORTS), len(_lib.RESP_EXPORTS), len(_lib.DET_EXPORTS), len(_lib.TOPUP_EXPORTS)) == \
        (52, 5, 6, 4, 3, 4), "the lists of the other headers are untouched"
    assert _lib.FAST_MASK_MODES == {"off": 0, "carried": 1}
    flat = " ".join(hdr.replace("*", " ").split())
    for what in ("a per-frame corner budget", "cv::circle-exact discs", "any change to votop_", "runByPixelsMask", "UNMASKED image",
                 "filtering afterwards is the wrong reading", "judged on the UNMASKED list"):
        assert what in flat, what   # the semantics and the out-of-scope list the header owes its reader
    for other in ("vo_topup.h", "vo_corners_mask.h"):   # ... and the two older headers point here
        assert "vo_fast_mask.h" in open(os.path.join(INC, other)).read(), other


def test_ctypes_structure_equals_the_headers_declaration():
    """vofm_params, declaration by declaration: the header's members in order, each an int, against the ctypes fields"""
    from visual_odom_amd import build, _lib
    build.build()
    hdr = open(os.path.join(INC, "vo_fast_mask.h")).read()
    body = re.search(r"typedef struct vofm_params \{(.*?)\} vofm_params;", hdr, re.S).group(1)
    members = re.findall(r"^\s*(\w+)\s+(\w+);", body, re.M)
    assert members == [("int", "mode"), ("int", "radius")]
    P = _lib.VoFmParams
    assert [(n, t) for n, t in P._fields_] == [(name, C.c_int) for _, name in members]
    assert C.sizeof(P) == 8 and (P.mode.offset, P.radius.offset) == (0, 4)
    p = P(9, 77)
    _lib.load().vofm_default_params(C.byref(p))
    assert (p.mode, p.radius) == (0, 5)   # VOFM_OFF, radius 5


def test_library_exports_the_fast_mask_names():
    from visual_odom_amd import build, _lib
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    defined = [l.split()[2] for l in out.splitlines() if len(l.split()) == 3 and l.split()[1] == "T"]
    assert sorted(s for s in defined if s.startswith("vofm")) == FM_NAMES
    assert sorted(s for s in defined if s.startswith("votop")) == sorted(_lib.TOPUP_EXPORTS)
    assert sorted(s for s in defined if s.startswith("vodet")) == sorted(_lib.DET_EXPORTS)
    lib = _lib.load()
    vp, i, prm = C.c_void_p, C.c_int, C.POINTER(_lib.VoFmParams)
    want = {"vofm_default_params": [prm], "vofm_set_params": [vp, prm], "vofm_get_params": [vp, prm], "vofm_get_mask": [vp, i, vp, i],
            "vofm_detect": [vp, vp, i, i, i, i, i, vp, i, vp, i, vp], "vofm_replenish": [vp, vp, i, i, i, i, i, vp, i, i, vp, i, vp]}
    for name in FM_NAMES:
        assert list(getattr(lib, name).argtypes) == want[name], name
        assert getattr(lib, name).restype is (None if name == "vofm_default_params" else C.c_int)
    blob = open(so, "rb").read()
    for kernel in (b"fast_mask_filter_kernel", b"corn_disc_frames_kernel", b"fast_nms_write_kernel", b"bucket_kernel"):
        assert kernel in blob, kernel
    assert "capi_fast_mask.hip" in build.SOURCES


def test_bad_calls_that_need_no_device():
    """a NULL context is VO_ERR_ARG in every entry point, whatever else the call says -- a NULL mask with a stride, a short stride, a
    radius of -1 or 257, mode 7, n_kept beyond any max_pts; the same table with a context is test_gpu_fast_mask.py's"""
    from visual_odom_amd import build, _lib
    build.build()
    lib = _lib.load()
    p = _lib.VoFmParams()
    buf = (C.c_uint8 * 64)()
    pts = (C.c_float * 8)()
    n = C.c_int(-9)
    E = _lib.VO_ERR_ARG
    assert lib.vofm_set_params(None, C.byref(p)) == E and lib.vofm_set_params(None, None) == E
    assert lib.vofm_set_params(None, C.byref(_lib.VoFmParams(7, 5))) == E
    assert lib.vofm_set_params(None, C.byref(_lib.VoFmParams(1, -1))) == E and lib.vofm_set_params(None, C.byref(_lib.VoFmParams(1, 257))) == E
    assert lib.vofm_get_params(None, C.byref(p)) == E
    assert lib.vofm_get_mask(None, 0, buf, 4) == E
    for mask, stride in ((None, 8), (buf, 4), (buf, 8), (None, 0)):
        assert lib.vofm_detect(None, buf, 8, 8, 8, 20, 1, mask, stride, pts, 4, C.byref(n)) == E
    for n_kept, radius in ((2, -1), (2, 257), (1 << 30, 5), (2, 5)):
        assert lib.vofm_replenish(None, buf, 8, 8, 8, 20, 1, pts, n_kept, radius, pts, 4, C.byref(n)) == E
    assert n.value == -9
    lib.vofm_default_params(None)   # (a NULL record is ignored)
