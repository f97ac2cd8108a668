"""include/vo_corners.h -- the fifth header, the Shi-Tomasi detector beside vo_hip.h: it compiles as C99 and as C++11, the ctypes
mirror lists exactly its names (_lib.CORN_EXPORTS), libvo_hip.so exports exactly them under the vocorn prefix and carries the
kernels, no other header mentions the prefix, the C ABI's own list is untouched, and every entry point refuses a NULL context.  No
compute calls."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
CORN_NAMES = ["vocorn_batch_get", "vocorn_batch_run", "vocorn_default_params", "vocorn_detect", "vocorn_min_eigen_map"]


def declared(header, prefix):
    hdr = open(os.path.join(INC, header)).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(%s[a-z0-9_]+)\s*\(" % prefix, hdr)))


def test_corners_header_compiles_as_c_and_cxx11(tmp_path):
    src = tmp_path / "use_corners.c"
    src.write_text('#include "vo_corners.h"\n'
                   "typedef char range[VOCORN_MAX_MIN_DISTANCE >= 32 ? 1 : -1];\n"
                   "int use(vo_ctx *c, const uint8_t *img, float *pts, float *eig, int *n)\n"
                   "{\n"
                   "    vocorn_params p;\n"
                   "    int rc;\n"
                   "    vocorn_default_params(&p);\n"
                   "    p.max_corners = 100;\n"
                   "    rc = vocorn_detect(c, img, 64, 48, 64, &p, pts, 100, n);\n"
                   "    rc |= vocorn_min_eigen_map(c, img, 64, 48, 64, eig, 64);\n"
                   "    rc |= vocorn_batch_run(c, &p, 0, 2) | vocorn_batch_get(c, 1, pts, 100, n);\n"
                   "    return rc == VO_OK ? 0 : VO_ERR_ARG;\n"
                   "}\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I" + INC, str(src)])
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", "-I" + INC, str(src)])


def test_corners_binding_list_matches_header():
    from visual_odom_amd import _lib
    assert declared("vo_corners.h", "vocorn_") == CORN_NAMES
    assert sorted(_lib.CORN_EXPORTS) == CORN_NAMES
    for prefix in ("vo_", "voflow", "vowin", "voflag"):
        assert declared("vo_corners.h", prefix) == [], "nothing under " + prefix
    others = set(_lib.EXPORTS) | set(_lib.FLOW_EXPORTS) | set(_lib.WIN_EXPORTS) | set(_lib.FLAG_EXPORTS)
    assert not set(_lib.CORN_EXPORTS) & others
    hdr = open(os.path.join(INC, "vo_corners.h")).read()
    assert '#include "vo_hip.h"' in hdr
    for other in ("vo_hip.h", "vo_flow.h", "vo_flow_win.h", "vo_flow_flags.h"):
        assert "vocorn" not in open(os.path.join(INC, other)).read().lower(), other
    assert len(_lib.EXPORTS) == 52, "the C ABI's own list is untouched"
    p = _lib.VoCornParams()
    _lib.load().vocorn_default_params(C.byref(p))
    assert (p.max_corners, p.quality_level, p.min_distance) == (5000, 0.01, 5.0)   # feature.cpp:53-55
    assert C.sizeof(_lib.VoCornParams) == 24


def test_library_exports_the_corner_names():
    from visual_odom_amd import build, _lib
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    syms = sorted(l.split()[2] for l in out.splitlines() if len(l.split()) == 3 and l.split()[1] == "T" and l.split()[2].startswith("vocorn"))
    assert syms == CORN_NAMES
    lib = _lib.load()
    for name in CORN_NAMES:
        assert getattr(lib, name).argtypes
        assert getattr(lib, name).restype is (None if name == "vocorn_default_params" else C.c_int)
    blob = open(so, "rb").read()
    for kernel in (b"corn_map_kernel", b"corn_cand_kernel", b"corn_select_kernel"):
        assert kernel in blob, kernel
    assert "corners.hip" in build.SOURCES and "capi_corners.hip" in build.SOURCES


def test_null_context_is_an_argument_error():
    from visual_odom_amd import build, _lib
    build.build()
    lib = _lib.load()
    p = _lib.VoCornParams(10, 0.01, 5.0)
    n = C.c_int(0)
    assert lib.vocorn_detect(None, None, 64, 48, 64, C.byref(p), None, 0, C.byref(n)) == _lib.VO_ERR_ARG
    assert lib.vocorn_min_eigen_map(None, None, 64, 48, 64, None, 64) == _lib.VO_ERR_ARG
    assert lib.vocorn_batch_run(None, C.byref(p), 0, 1) == _lib.VO_ERR_ARG
    assert lib.vocorn_batch_get(None, 0, None, 0, C.byref(n)) == _lib.VO_ERR_ARG
    lib.vocorn_default_params(None)   # (a NULL record is ignored)
