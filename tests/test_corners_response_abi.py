"""include/vo_corners_response.h -- the seventh header, goodFeaturesToTrack's blockSize / useHarrisDetector / k beside vo_corners.h and
vo_corners_mask.h: it compiles as C99 and as C++11, the ctypes mirror lists exactly its names (_lib.RESP_EXPORTS), libvo_hip.so
exports exactly them under the voresp prefix and carries the kernels, the other prefixes and lists are untouched, and every entry
point refuses a NULL context.  No compute calls."""
import ctypes as C
import os
import subprocess

from test_corners_abi import INC, declared

RESP_NAMES = ["voresp_batch_run", "voresp_default_params", "voresp_detect", "voresp_map"]


def test_response_header_compiles_as_c_and_cxx11(tmp_path):
    src = tmp_path / "use_corners_response.c"
    src.write_text('#include "vo_corners_response.h"\n'
                   "typedef char size16[sizeof(voresp_params) == 16 ? 1 : -1];\n"
                   "int use(vo_ctx *c, const uint8_t *img, const uint8_t *mask, const float *kept, float *pts, float *map, int *n)\n"
                   "{\n"
                   "    vocorn_params p;\n"
                   "    voresp_params r;\n"
                   "    int rc;\n"
                   "    vocorn_default_params(&p);\n"
                   "    voresp_default_params(&r);\n"
                   "    r.block_size = 5;\n"
                   "    r.use_harris = 1;\n"
                   "    r.k = 0.06;\n"
                   "    rc = voresp_map(c, img, 64, 48, 64, &r, map, 64);\n"
                   "    rc |= voresp_detect(c, img, 64, 48, 64, mask, 64, &p, &r, pts, 100, n);\n"
                   "    rc |= vocmask_batch_set_kept(c, 1, kept, 10, 5);\n"
                   "    rc |= voresp_batch_run(c, &p, &r, 0, 2) | vocorn_batch_get(c, 1, pts, 100, n);\n"
                   "    return rc == VO_OK ? 0 : VO_ERR_ARG;\n"
                   "}\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I" + INC, str(src)])
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", "-I" + INC, str(src)])


def test_response_binding_list_matches_header():
    from visual_odom_amd import _lib
    assert declared("vo_corners_response.h", "voresp_") == RESP_NAMES
    assert sorted(_lib.RESP_EXPORTS) == RESP_NAMES
    for prefix in ("vo_", "voflow", "vowin", "voflag", "vocorn", "vocmask"):
        assert declared("vo_corners_response.h", prefix) == [], "nothing under " + prefix
    others = (set(_lib.EXPORTS) | set(_lib.FLOW_EXPORTS) | set(_lib.WIN_EXPORTS) | set(_lib.FLAG_EXPORTS) | set(_lib.CORN_EXPORTS) |
              set(_lib.CMASK_EXPORTS))
    assert not set(_lib.RESP_EXPORTS) & others
    hdr = open(os.path.join(INC, "vo_corners_response.h")).read()
    assert '#include "vo_corners_mask.h"' in hdr
    for other in ("vo_hip.h", "vo_flow.h", "vo_flow_win.h", "vo_flow_flags.h", "vo_corners.h", "vo_corners_mask.h"):
        assert declared(other, "voresp") == [], other + " declares nothing under the new prefix"
    assert len(_lib.EXPORTS) == 52 and len(_lib.CORN_EXPORTS) == 5 and len(_lib.CMASK_EXPORTS) == 6, "the lists of the other headers are untouched"
    p = _lib.VoRespParams()
    _lib.load().voresp_default_params(C.byref(p))
    assert (p.block_size, p.use_harris, p.k) == (3, 0, 0.04)   # cv::goodFeaturesToTrack's defaults
    assert C.sizeof(_lib.VoRespParams) == 16


def test_library_exports_the_response_names():
    from visual_odom_amd import build, _lib
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    syms = sorted(l.split()[2] for l in out.splitlines() if len(l.split()) == 3 and l.split()[1] == "T" and l.split()[2].startswith("voresp"))
    assert syms == RESP_NAMES
    lib = _lib.load()
    vp, i, prm, rsp = C.c_void_p, C.c_int, C.POINTER(_lib.VoCornParams), C.POINTER(_lib.VoRespParams)
    want = {"voresp_default_params": [rsp], "voresp_map": [vp, vp, i, i, i, rsp, vp, i], "voresp_detect": [vp, vp, i, i, i, vp, i, prm, rsp, vp, i, vp],
            "voresp_batch_run": [vp, prm, rsp, i, i]}
    for name in RESP_NAMES:
        assert list(getattr(lib, name).argtypes) == want[name], name
        assert getattr(lib, name).restype is (None if name == "voresp_default_params" else C.c_int)
    blob = open(so, "rb").read()
    for kernel in (b"corn_map_resp_kernelILi5ELi0EE", b"corn_map_resp_kernelILi3ELi1EE", b"corn_map_resp_kernelILi5ELi1EE", b"corn_map_kernel",
                   b"corn_map_masked_kernel", b"corn_cand_kernel", b"corn_select_kernel", b"corn_disc_kernel"):
        assert kernel in blob, kernel
    assert "capi_corners_response.hip" in build.SOURCES


def test_null_context_is_an_argument_error():
    from visual_odom_amd import build, _lib
    build.build()
    lib = _lib.load()
    p, r = _lib.VoCornParams(10, 0.01, 5.0), _lib.VoRespParams(5, 1, 0.04)
    n = C.c_int(0)
    assert lib.voresp_map(None, None, 64, 48, 64, C.byref(r), None, 64) == _lib.VO_ERR_ARG
    assert lib.voresp_detect(None, None, 64, 48, 64, None, 64, C.byref(p), C.byref(r), None, 0, C.byref(n)) == _lib.VO_ERR_ARG
    assert lib.voresp_batch_run(None, C.byref(p), C.byref(r), 0, 1) == _lib.VO_ERR_ARG
    lib.voresp_default_params(None)   # (a NULL record is ignored)
