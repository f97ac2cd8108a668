"""include/vo_detector.h -- the eighth header, the frame loop's detector: it compiles as C99 and as C++11, the ctypes mirror lists
exactly its names (_lib.DET_EXPORTS) and lays vodet_params out as the C struct, libvo_hip.so exports exactly them under the vodet
prefix and carries the frames-form kernels, the other prefixes and lists are untouched, and every entry point refuses a NULL context.
No compute calls."""
import ctypes as C
import os
import subprocess

from test_corners_abi import INC, declared

DET_NAMES = ["vodet_default_params", "vodet_get_params", "vodet_set_params"]


def test_detector_header_compiles_as_c_and_cxx11(tmp_path):
    src = tmp_path / "use_detector.c"
    src.write_text('#include <stddef.h>\n#include "vo_detector.h"\n'
                   "typedef char size48[sizeof(vodet_params) == 48 ? 1 : -1];\n"
                   "typedef char off_c[offsetof(vodet_params, corners) == 8 ? 1 : -1];\n"
                   "typedef char off_r[offsetof(vodet_params, response) == 32 ? 1 : -1];\n"
                   "int use(vo_ctx *c, const uint8_t *img, float *pts, int32_t *ages, int *n)\n"
                   "{\n"
                   "    vodet_params p;\n"
                   "    int rc;\n"
                   "    vodet_default_params(&p);\n"
                   "    p.detector = VODET_SHI_TOMASI;\n"
                   "    p.corners.max_corners = 1000;\n"
                   "    p.response.block_size = 5;\n"
                   "    rc = vodet_set_params(c, &p) | vodet_get_params(c, &p);\n"
                   "    rc |= vo_detect_bucket(c, img, 64, 48, 64, NULL, pts, n, ages, n, 100);\n"
                   "    rc |= vodet_set_params(c, NULL);\n"
                   "    return rc == VO_OK && p.detector != VODET_FAST ? 0 : VO_ERR_ARG;\n"
                   "}\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I" + INC, str(src)])
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", "-I" + INC, str(src)])


def test_detector_binding_list_matches_header():
    from visual_odom_amd import _lib
    assert declared("vo_detector.h", "vodet_") == DET_NAMES
    assert sorted(_lib.DET_EXPORTS) == DET_NAMES
    for prefix in ("vo_", "voflow", "vowin", "voflag", "vocorn", "vocmask", "voresp"):
        assert declared("vo_detector.h", prefix) == [], "nothing under " + prefix
    others = (set(_lib.EXPORTS) | set(_lib.FLOW_EXPORTS) | set(_lib.WIN_EXPORTS) | set(_lib.FLAG_EXPORTS) | set(_lib.CORN_EXPORTS) |
              set(_lib.CMASK_EXPORTS) | set(_lib.RESP_EXPORTS))
    assert not set(_lib.DET_EXPORTS) & others
    hdr = open(os.path.join(INC, "vo_detector.h")).read()
    assert '#include "vo_corners_response.h"' in hdr
    for other in ("vo_hip.h", "vo_flow.h", "vo_flow_win.h", "vo_flow_flags.h", "vo_corners.h", "vo_corners_mask.h", "vo_corners_response.h"):
        assert declared(other, "vodet") == [], other + " declares nothing under the new prefix"
    assert len(_lib.EXPORTS) == 52 and len(_lib.CORN_EXPORTS) == 5 and len(_lib.CMASK_EXPORTS) == 6 and len(_lib.RESP_EXPORTS) == 4, \
        "the lists of the other headers are untouched"
    assert _lib.DETECTORS == {"fast": 0, "shi_tomasi": 1}


def test_params_layout_and_defaults():
    from visual_odom_amd import build, _lib
    build.build()
    P = _lib.VoDetParams
    assert C.sizeof(P) == 48 and (P.detector.offset, P.corners.offset, P.response.offset) == (0, 8, 32)
    assert C.sizeof(_lib.VoCornParams) == 24 and C.sizeof(_lib.VoRespParams) == 16
    p = P(9, _lib.VoCornParams(1, 2.0, 3.0), _lib.VoRespParams(5, 1, 9.0))
    _lib.load().vodet_default_params(C.byref(p))
    assert p.detector == 0                                                                       # VODET_FAST
    assert (p.corners.max_corners, p.corners.quality_level, p.corners.min_distance) == (5000, 0.01, 5.0)   # vocorn_default_params
    assert (p.response.block_size, p.response.use_harris, p.response.k) == (3, 0, 0.04)          # voresp_default_params


def test_library_exports_the_detector_names():
    from visual_odom_amd import build, _lib
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    syms = sorted(l.split()[2] for l in out.splitlines() if len(l.split()) == 3 and l.split()[1] == "T" and l.split()[2].startswith("vodet"))
    assert syms == DET_NAMES
    lib = _lib.load()
    vp, prm = C.c_void_p, C.POINTER(_lib.VoDetParams)
    want = {"vodet_default_params": [prm], "vodet_set_params": [vp, prm], "vodet_get_params": [vp, prm]}
    for name in DET_NAMES:
        assert list(getattr(lib, name).argtypes) == want[name], name
        assert getattr(lib, name).restype is (None if name == "vodet_default_params" else C.c_int)
    blob = open(so, "rb").read()
    for kernel in (b"corn_map_frames_kernelILi3ELi0EE", b"corn_map_frames_kernelILi5ELi0EE", b"corn_map_frames_kernelILi3ELi1EE",
                   b"corn_map_frames_kernelILi5ELi1EE", b"corn_cand_frames_kernel", b"corn_select_frames_kernel", b"corn_map_kernel",
                   b"corn_cand_kernel", b"corn_select_kernel"):
        assert kernel in blob, kernel
    assert "capi_detector.hip" in build.SOURCES


def test_null_context_is_an_argument_error():
    from visual_odom_amd import build, _lib
    build.build()
    lib = _lib.load()
    p = _lib.VoDetParams()
    assert lib.vodet_set_params(None, C.byref(p)) == _lib.VO_ERR_ARG
    assert lib.vodet_get_params(None, C.byref(p)) == _lib.VO_ERR_ARG
    lib.vodet_default_params(None)   # (a NULL record is ignored)
