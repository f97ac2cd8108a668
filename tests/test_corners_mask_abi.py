"""include/vo_corners_mask.h -- the sixth header, the Shi-Tomasi detector's mask argument beside vo_corners.h: it compiles as C99 and
as C++11, the ctypes mirror lists exactly its names (_lib.CMASK_EXPORTS), libvo_hip.so exports exactly them under the vocmask prefix
and carries the kernels, the other prefixes and lists are untouched, and every entry point refuses a NULL context.  No compute
calls."""
import ctypes as C
import os
import subprocess

from test_corners_abi import INC, declared

CMASK_NAMES = ["vocmask_batch_run", "vocmask_batch_set_kept", "vocmask_batch_set_mask", "vocmask_detect", "vocmask_disc_mask", "vocmask_replenish"]


def test_mask_header_compiles_as_c_and_cxx11(tmp_path):
    src = tmp_path / "use_corners_mask.c"
    src.write_text('#include "vo_corners_mask.h"\n'
                   "int use(vo_ctx *c, const uint8_t *img, const uint8_t *mask, uint8_t *mask_out, const float *kept, float *pts, int *n)\n"
                   "{\n"
                   "    vocorn_params p;\n"
                   "    int rc;\n"
                   "    vocorn_default_params(&p);\n"
                   "    p.max_corners = 100;\n"
                   "    rc = vocmask_detect(c, img, 64, 48, 64, mask, 64, &p, pts, 100, n);\n"
                   "    rc |= vocmask_disc_mask(c, 64, 48, kept, 10, 5, mask_out, 64);\n"
                   "    rc |= vocmask_replenish(c, img, 64, 48, 64, kept, 10, 5, &p, pts, 100, n);\n"
                   "    rc |= vocmask_batch_set_mask(c, 0, mask, 64) | vocmask_batch_set_kept(c, 1, kept, 10, VOCORN_MAX_MIN_DISTANCE);\n"
                   "    rc |= vocmask_batch_run(c, &p, 0, 2) | vocorn_batch_get(c, 1, pts, 100, n);\n"
                   "    return rc == VO_OK ? 0 : VO_ERR_ARG;\n"
                   "}\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I" + INC, str(src)])
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", "-I" + INC, str(src)])


def test_mask_binding_list_matches_header():
    from visual_odom_amd import _lib
    assert declared("vo_corners_mask.h", "vocmask_") == CMASK_NAMES
    assert sorted(_lib.CMASK_EXPORTS) == CMASK_NAMES
    for prefix in ("vo_", "voflow", "vowin", "voflag", "vocorn"):
        assert declared("vo_corners_mask.h", prefix) == [], "nothing under " + prefix
    others = set(_lib.EXPORTS) | set(_lib.FLOW_EXPORTS) | set(_lib.WIN_EXPORTS) | set(_lib.FLAG_EXPORTS) | set(_lib.CORN_EXPORTS)
    assert not set(_lib.CMASK_EXPORTS) & others
    hdr = open(os.path.join(INC, "vo_corners_mask.h")).read()
    assert '#include "vo_corners.h"' in hdr
    for other in ("vo_hip.h", "vo_flow.h", "vo_flow_win.h", "vo_flow_flags.h"):
        assert "vocmask" not in open(os.path.join(INC, other)).read().lower(), other
    assert len(_lib.EXPORTS) == 52 and len(_lib.CORN_EXPORTS) == 5, "the lists of the other headers are untouched"


def test_library_exports_the_mask_names():
    from visual_odom_amd import build, _lib
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    syms = sorted(l.split()[2] for l in out.splitlines() if len(l.split()) == 3 and l.split()[1] == "T" and l.split()[2].startswith("vocmask"))
    assert syms == CMASK_NAMES
    lib = _lib.load()
    vp, i, prm = C.c_void_p, C.c_int, C.POINTER(_lib.VoCornParams)
    want = {"vocmask_detect": [vp, vp, i, i, i, vp, i, prm, vp, i, vp], "vocmask_disc_mask": [vp, i, i, vp, i, i, vp, i],
            "vocmask_replenish": [vp, vp, i, i, i, vp, i, i, prm, vp, i, vp], "vocmask_batch_set_mask": [vp, i, vp, i],
            "vocmask_batch_set_kept": [vp, i, vp, i, i], "vocmask_batch_run": [vp, prm, i, i]}
    for name in CMASK_NAMES:
        assert list(getattr(lib, name).argtypes) == want[name], name
        assert getattr(lib, name).restype is C.c_int
    blob = open(so, "rb").read()
    for kernel in (b"corn_map_kernel", b"corn_map_masked_kernel", b"corn_cand_kernel", b"corn_select_kernel", b"corn_disc_kernel"):
        assert kernel in blob, kernel
    assert "capi_corners_mask.hip" in build.SOURCES


def test_null_context_is_an_argument_error():
    from visual_odom_amd import build, _lib
    build.build()
    lib = _lib.load()
    p = _lib.VoCornParams(10, 0.01, 5.0)
    n = C.c_int(0)
    assert lib.vocmask_detect(None, None, 64, 48, 64, None, 64, C.byref(p), None, 0, C.byref(n)) == _lib.VO_ERR_ARG
    assert lib.vocmask_disc_mask(None, 64, 48, None, 0, 5, None, 64) == _lib.VO_ERR_ARG
    assert lib.vocmask_replenish(None, None, 64, 48, 64, None, 0, 5, C.byref(p), None, 0, C.byref(n)) == _lib.VO_ERR_ARG
    assert lib.vocmask_batch_set_mask(None, 0, None, 64) == _lib.VO_ERR_ARG
    assert lib.vocmask_batch_set_kept(None, 0, None, 0, 5) == _lib.VO_ERR_ARG
    assert lib.vocmask_batch_run(None, C.byref(p), 0, 1) == _lib.VO_ERR_ARG
