"""include/vo_flow_flags.h -- the flags header beside vo_flow_win.h: it compiles as C99 and as C++11, the ctypes mirror lists exactly
its names (_lib.FLAG_EXPORTS) and its two constants, libvo_hip.so exports exactly them under the voflag prefix and carries the nine
kernels, the header declares nothing under vo_, voflow or vowin, and every entry point refuses a NULL context.  No compute calls."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
FLAG_NAMES = ["voflag_batch_run", "voflag_batch_set_guess", "voflag_feature_tracking", "voflag_track"]


def declared(header, prefix):
    hdr = open(os.path.join(INC, header)).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(%s[a-z0-9_]+)\s*\(" % prefix, hdr)))


def test_flags_header_compiles_as_c_and_cxx11(tmp_path):
    src = tmp_path / "use_flags.c"
    src.write_text('#include "vo_flow_flags.h"\n'
                   "typedef char four[VOFLAG_USE_INITIAL_FLOW == 4 ? 1 : -1];\n"
                   "typedef char eight[VOFLAG_GET_MIN_EIGENVALS == 8 ? 1 : -1];\n"
                   "int use(vo_ctx *c, const uint8_t *a, const uint8_t *b, float *p, uint8_t *s, int32_t *k, int *n)\n"
                   "{\n"
                   "    int rc = voflag_track(c, a, b, 64, 48, 64, p, 1, 15, VOFLAG_USE_INITIAL_FLOW, p, s, 0);\n"
                   "    rc |= voflag_feature_tracking(c, a, b, 64, 48, 64, p, 1, 7, VOFLAG_USE_INITIAL_FLOW | VOFLAG_GET_MIN_EIGENVALS, p, s, p, k, n);\n"
                   "    rc |= voflow_batch_set_pairs(c, k, 1) | voflag_batch_set_guess(c, 0, p, 1) | voflag_batch_run(c, 9, VOFLAG_GET_MIN_EIGENVALS);\n"
                   "    rc |= voflow_batch_get(c, 0, p, s, p, 1) | vowin_max_level(c, 64, 48, n);\n"
                   "    return rc == VO_OK ? 0 : VO_ERR_ARG;\n"
                   "}\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I" + INC, str(src)])
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", "-I" + INC, str(src)])


def test_flags_binding_list_matches_header():
    from visual_odom_amd import _lib
    assert declared("vo_flow_flags.h", "voflag_") == FLAG_NAMES
    assert sorted(_lib.FLAG_EXPORTS) == FLAG_NAMES
    for prefix in ("vo_", "voflow", "vowin"):
        assert declared("vo_flow_flags.h", prefix) == [], "nothing under " + prefix
    assert not set(_lib.FLAG_EXPORTS) & (set(_lib.EXPORTS) | set(_lib.FLOW_EXPORTS) | set(_lib.WIN_EXPORTS))
    hdr = open(os.path.join(INC, "vo_flow_flags.h")).read()
    assert '#include "vo_flow_win.h"' in hdr
    assert re.search(r"#define\s+VOFLAG_USE_INITIAL_FLOW\s+4\b", hdr) and re.search(r"#define\s+VOFLAG_GET_MIN_EIGENVALS\s+8\b", hdr)
    assert (_lib.FLAG_USE_INITIAL_FLOW, _lib.FLAG_GET_MIN_EIGENVALS) == (4, 8)
    for other in ("vo_hip.h", "vo_flow.h", "vo_flow_win.h"):
        assert "voflag" not in open(os.path.join(INC, other)).read().lower(), other
    assert len(_lib.EXPORTS) == 52, "the C ABI's own list is untouched"


def test_library_exports_the_flag_names():
    from visual_odom_amd import build, _lib
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    syms = sorted(l.split()[2] for l in out.splitlines() if len(l.split()) == 3 and l.split()[1] == "T" and l.split()[2].startswith("voflag"))
    assert syms == FLAG_NAMES
    lib = _lib.load()
    for name in FLAG_NAMES:
        assert getattr(lib, name).restype is C.c_int and getattr(lib, name).argtypes
    blob = open(so, "rb").read()
    for w in (5, 7, 9, 11, 13, 15, 17, 19, 21):   # one instantiation per window, 21 included (Itanium mangling: ILi<W>E)
        assert b"lk_flow_flags_kernelILi%dE" % w in blob, w


def test_null_context_is_an_argument_error():
    from visual_odom_amd import build, _lib
    build.build()
    lib = _lib.load()
    assert lib.voflag_track(None, None, None, 64, 48, 64, None, 0, 15, 4, None, None, None) == _lib.VO_ERR_ARG
    assert lib.voflag_feature_tracking(None, None, None, 64, 48, 64, None, 0, 15, 8, None, None, None, None, None) == _lib.VO_ERR_ARG
    assert lib.voflag_batch_set_guess(None, 0, None, 0) == _lib.VO_ERR_ARG
    assert lib.voflag_batch_run(None, 15, 4) == _lib.VO_ERR_ARG
