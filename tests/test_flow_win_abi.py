"""include/vo_flow_win.h -- the windowed tracker's header beside vo_flow.h: it compiles as C99 and as C++11, the ctypes mirror lists
exactly its names (_lib.WIN_EXPORTS), libvo_hip.so exports exactly them under the vowin prefix and carries the windowed kernels,
the header declares nothing under vo_ or voflow, and every entry point refuses a NULL context.  No compute calls here."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
WIN_NAMES = ["vowin_batch_run", "vowin_feature_tracking", "vowin_max_level", "vowin_track"]


def declared(header, prefix):
    hdr = open(os.path.join(INC, header)).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(%s[a-z0-9_]+)\s*\(" % prefix, hdr)))


def test_win_header_compiles_as_c_and_cxx11(tmp_path):
    src = tmp_path / "use_win.c"
    src.write_text('#include "vo_flow_win.h"\n'
                   "int use(vo_ctx *c, const uint8_t *a, const uint8_t *b, float *p, uint8_t *s, int32_t *k, int *n)\n"
                   "{\n"
                   "    int rc = vowin_track(c, a, b, 64, 48, 64, p, 1, 15, p, s, 0);\n"
                   "    rc |= vowin_feature_tracking(c, a, b, 64, 48, 64, p, 1, 7, p, s, p, k, n);\n"
                   "    rc |= voflow_batch_set_pairs(c, k, 1) | vowin_batch_run(c, 9) | voflow_batch_get(c, 0, p, s, p, 1);\n"
                   "    rc |= vowin_max_level(c, 64, 48, n);\n"
                   "    return rc == VO_OK ? 0 : VO_ERR_ARG;\n"
                   "}\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I" + INC, str(src)])
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", "-I" + INC, str(src)])


def test_win_binding_list_matches_header():
    from visual_odom_amd import _lib
    assert declared("vo_flow_win.h", "vowin_") == WIN_NAMES
    assert sorted(_lib.WIN_EXPORTS) == WIN_NAMES
    assert declared("vo_flow_win.h", "vo_") == [] and declared("vo_flow_win.h", "voflow") == [], "nothing under vo_ or voflow"
    assert not set(_lib.WIN_EXPORTS) & (set(_lib.EXPORTS) | set(_lib.FLOW_EXPORTS))
    assert '#include "vo_flow.h"' in open(os.path.join(INC, "vo_flow_win.h")).read()
    assert "vowin" not in open(os.path.join(INC, "vo_flow.h")).read() and "vowin" not in open(os.path.join(INC, "vo_hip.h")).read()


def test_library_exports_the_win_names():
    from visual_odom_amd import build, _lib
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    syms = sorted(l.split()[2] for l in out.splitlines() if len(l.split()) == 3 and l.split()[1] == "T" and l.split()[2].startswith("vowin"))
    assert syms == WIN_NAMES
    lib = _lib.load()
    for name in WIN_NAMES:
        assert getattr(lib, name).restype is C.c_int and getattr(lib, name).argtypes
    blob = open(so, "rb").read()
    assert b"lk_flow_win_kernel" in blob
    for w in (5, 7, 9, 11, 13, 15, 17, 19):   # one instantiation per window (Itanium mangling: template argument ILi<W>E)
        assert b"lk_flow_win_kernelILi%dE" % w in blob, w
    assert b"lk_flow_win_kernelILi21E" not in blob, "21 is lk_flow_kernel"


def test_null_context_is_an_argument_error():
    from visual_odom_amd import build, _lib
    build.build()
    lib = _lib.load()
    e = C.c_int(-7)
    assert lib.vowin_track(None, None, None, 64, 48, 64, None, 0, 15, None, None, None) == _lib.VO_ERR_ARG
    assert lib.vowin_feature_tracking(None, None, None, 64, 48, 64, None, 0, 15, None, None, None, None, None) == _lib.VO_ERR_ARG
    assert lib.vowin_batch_run(None, 15) == _lib.VO_ERR_ARG
    assert lib.vowin_max_level(None, 64, 48, C.addressof(e)) == _lib.VO_ERR_ARG and e.value == -7
