"""include/vo_topup.h -- the ninth header, the frame loop's top-up under a mask of the carried points: it compiles as C99 and as C++11,
the ctypes mirror lists exactly its names (_lib.TOPUP_EXPORTS) and lays votop_params out as the C struct, libvo_hip.so exports exactly
them under the votop prefix and carries the new kernels, the other prefixes and lists are untouched (vodet_params stays 48 bytes,
vo_detector.h declares nothing new), and every entry point refuses a NULL context.  No compute calls."""
import ctypes as C
import os
import subprocess

from test_corners_abi import INC, declared

TOP_NAMES = ["votop_default_params", "votop_get_mask", "votop_get_params", "votop_set_params"]
OTHER_PREFIXES = ("vo_", "voflow", "vowin", "voflag", "vocorn", "vocmask", "voresp", "vodet")
OTHER_HEADERS = ("vo_hip.h", "vo_flow.h", "vo_flow_win.h", "vo_flow_flags.h", "vo_corners.h", "vo_corners_mask.h", "vo_corners_response.h", "vo_detector.h")


def test_topup_header_compiles_as_c_and_cxx11(tmp_path):
    src = tmp_path / "use_topup.c"
    src.write_text('#include <stddef.h>\n#include "vo_topup.h"\n'
                   "typedef char size8[sizeof(votop_params) == 8 ? 1 : -1];\n"
                   "typedef char off_m[offsetof(votop_params, mode) == 0 ? 1 : -1];\n"
                   "typedef char off_r[offsetof(votop_params, radius) == 4 ? 1 : -1];\n"
                   "typedef char det48[sizeof(vodet_params) == 48 ? 1 : -1];\n"
                   "typedef char modes[VOTOP_OFF == 0 && VOTOP_CARRIED == 1 ? 1 : -1];\n"
                   "int use(vo_ctx *c, const uint8_t *img, float *pts, int32_t *ages, int *n, uint8_t *mask)\n"
                   "{\n"
                   "    votop_params p;\n"
                   "    vodet_params d;\n"
                   "    int rc;\n"
                   "    votop_default_params(&p);\n"
                   "    vodet_default_params(&d);\n"
                   "    d.detector = VODET_SHI_TOMASI;\n"
                   "    p.mode = VOTOP_CARRIED;\n"
                   "    p.radius = VOCORN_MAX_MIN_DISTANCE;\n"
                   "    rc = vodet_set_params(c, &d) | votop_set_params(c, &p) | votop_get_params(c, &p);\n"
                   "    rc |= vo_detect_bucket(c, img, 64, 48, 64, NULL, pts, n, ages, n, 100);\n"
                   "    rc |= votop_get_mask(c, 0, mask, 64);\n"
                   "    rc |= votop_set_params(c, NULL);\n"
                   "    return rc == VO_OK && p.mode != VOTOP_OFF ? 0 : VO_ERR_ARG;\n"
                   "}\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I" + INC, str(src)])
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", "-I" + INC, str(src)])


def test_topup_binding_list_matches_header():
    from visual_odom_amd import _lib
    assert declared("vo_topup.h", "votop_") == TOP_NAMES
    assert sorted(_lib.TOPUP_EXPORTS) == TOP_NAMES
    for prefix in OTHER_PREFIXES:
        assert declared("vo_topup.h", prefix) == [], "nothing under " + prefix
        assert not "votop".startswith(prefix) and not prefix.startswith("votop")
    others = (set(_lib.EXPORTS) | set(_lib.FLOW_EXPORTS) | set(_lib.WIN_EXPORTS) | set(_lib.FLAG_EXPORTS) | set(_lib.CORN_EXPORTS) |
              set(_lib.CMASK_EXPORTS) | set(_lib.RESP_EXPORTS) | set(_lib.DET_EXPORTS))
    assert not set(_lib.TOPUP_EXPORTS) & others
    hdr = open(os.path.join(INC, "vo_topup.h")).read()
    assert '#include "vo_detector.h"' in hdr
    for other in OTHER_HEADERS:
        assert declared(other, "votop") == [], other + " declares nothing under the new prefix"
    assert declared("vo_detector.h", "vodet_") == ["vodet_default_params", "vodet_get_params", "vodet_set_params"]
    assert (len(_lib.EXPORTS), len(_lib.CORN_EXPORTS), len(_lib.CMASK_EXPORTS), len(_lib.RESP_EXPORTS), len(_lib.DET_EXPORTS)) == (52, 5, 6, 4, 3), \
        "the lists of the other headers are untouched"
    assert _lib.TOPUP_MODES == {"off": 0, "carried": 1}
    for what in ("a per-frame corner budget", "cv::circle-exact discs", "a mask for cv::FAST", "a latency form of the map pass"):
        assert what in " ".join(hdr.replace("*", " ").split()), what   # the out-of-scope list names what is still left
    for other in ("vo_detector.h", "vo_corners_mask.h"):                # ... and the two older headers point here instead
        text = open(os.path.join(INC, other)).read()
        assert "vo_topup.h" in text and "masks in the frame loop" not in text, other


def test_params_layout_and_defaults():
    from visual_odom_amd import build, _lib
    build.build()
    P = _lib.VoTopParams
    assert C.sizeof(P) == 8 and (P.mode.offset, P.radius.offset) == (0, 4)
    assert C.sizeof(_lib.VoDetParams) == 48
    p = P(9, 77)
    _lib.load().votop_default_params(C.byref(p))
    assert (p.mode, p.radius) == (0, 5)   # VOTOP_OFF, radius 5


def test_library_exports_the_topup_names():
    from visual_odom_amd import build, _lib
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    defined = [l.split()[2] for l in out.splitlines() if len(l.split()) == 3 and l.split()[1] == "T"]
    assert sorted(s for s in defined if s.startswith("votop")) == TOP_NAMES
    assert sorted(s for s in defined if s.startswith("vodet")) == sorted(_lib.DET_EXPORTS)
    assert sorted(s for s in defined if s.startswith("vocmask")) == sorted(_lib.CMASK_EXPORTS)
    lib = _lib.load()
    vp, i, prm = C.c_void_p, C.c_int, C.POINTER(_lib.VoTopParams)
    want = {"votop_default_params": [prm], "votop_set_params": [vp, prm], "votop_get_params": [vp, prm], "votop_get_mask": [vp, i, vp, i]}
    for name in TOP_NAMES:
        assert list(getattr(lib, name).argtypes) == want[name], name
        assert getattr(lib, name).restype is (None if name == "votop_default_params" else C.c_int)
    blob = open(so, "rb").read()
    for kernel in (b"corn_disc_frames_kernel", b"corn_max_frames_kernel", b"corn_disc_kernel", b"corn_map_frames_kernelILi3ELi0EE",
                   b"corn_map_frames_kernelILi5ELi1EE", b"corn_cand_frames_kernel", b"corn_select_frames_kernel"):
        assert kernel in blob, kernel
    assert "capi_topup.hip" in build.SOURCES


def test_null_context_is_an_argument_error():
    from visual_odom_amd import build, _lib
    build.build()
    lib = _lib.load()
    p = _lib.VoTopParams()
    buf = (C.c_uint8 * 16)()
    assert lib.votop_set_params(None, C.byref(p)) == _lib.VO_ERR_ARG
    assert lib.votop_get_params(None, C.byref(p)) == _lib.VO_ERR_ARG
    assert lib.votop_get_mask(None, 0, buf, 4) == _lib.VO_ERR_ARG
    lib.votop_default_params(None)   # (a NULL record is ignored)
