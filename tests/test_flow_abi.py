"""include/vo_flow.h -- the two-image tracker's header beside the C ABI: it compiles as C and as C++11, the ctypes mirror lists
exactly its names (_lib.FLOW_EXPORTS), libvo_hip.so exports exactly them under the voflow_ prefix, and the ABI of vo_hip.h is
what it was: no voflow_ name in it, _lib.EXPORTS unchanged, vo_params not grown.  No compute calls here."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
FLOW_NAMES = ["voflow_batch_get", "voflow_batch_run", "voflow_batch_set_pairs", "voflow_feature_tracking", "voflow_track"]


def declared(header, prefix):
    hdr = open(os.path.join(INC, header)).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(%s[a-z0-9_]+)\s*\(" % prefix, hdr)))


def test_flow_header_compiles_as_c_and_cxx11(tmp_path):
    src = tmp_path / "use_flow.c"
    src.write_text('#include "vo_flow.h"\n'
                   "int use(vo_ctx *c, const uint8_t *a, const uint8_t *b, float *p, uint8_t *s, int32_t *k, int *n)\n"
                   "{\n"
                   "    int rc = voflow_track(c, a, b, 64, 48, 64, p, 1, p, s, 0);\n"
                   "    rc |= voflow_feature_tracking(c, a, b, 64, 48, 64, p, 1, p, s, p, k, n);\n"
                   "    rc |= voflow_batch_set_pairs(c, k, 1) | voflow_batch_run(c) | voflow_batch_get(c, 0, p, s, p, 1);\n"
                   "    return rc == VO_OK ? 0 : VO_ERR_ARG;\n"
                   "}\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I" + INC, str(src)])
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", "-I" + INC, str(src)])


def test_flow_binding_list_matches_header():
    from visual_odom_amd import _lib
    assert declared("vo_flow.h", "voflow_") == FLOW_NAMES
    assert sorted(_lib.FLOW_EXPORTS) == FLOW_NAMES
    assert declared("vo_flow.h", "vo_") == [], "the new header declares nothing under the vo_ prefix"


def test_library_exports_the_flow_names():
    from visual_odom_amd import build, _lib
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    syms = sorted(l.split()[2] for l in out.splitlines() if len(l.split()) == 3 and l.split()[1] == "T" and l.split()[2].startswith("voflow"))
    assert syms == FLOW_NAMES
    lib = _lib.load()
    for name in FLOW_NAMES:
        assert getattr(lib, name).restype is C.c_int and getattr(lib, name).argtypes
    blob = open(so, "rb").read()
    assert b"lk_flow_kernel" in blob and b"flow_compact_kernel" in blob


def test_the_abi_of_vo_hip_h_is_what_it_was(tmp_path):
    from visual_odom_amd import _lib
    assert declared("vo_hip.h", "voflow_") == [] and "vo_flow" not in open(os.path.join(INC, "vo_hip.h")).read()
    assert len(_lib.EXPORTS) == 52 and sorted(_lib.EXPORTS) == declared("vo_hip.h", "vo_")
    assert not set(_lib.EXPORTS) & set(_lib.FLOW_EXPORTS)
    src = tmp_path / "size.c"
    src.write_text('#include "vo_flow.h"\n#include <stdio.h>\nint main(void) { printf("%d\\n", (int)sizeof(vo_params)); return 0; }\n')
    exe = str(tmp_path / "size")
    subprocess.check_call(["gcc", "-std=c99", "-I" + INC, str(src), "-o", exe])
    assert int(subprocess.check_output([exe])) == 128 == C.sizeof(_lib.VoParams)


def test_null_context_is_an_argument_error():
    """the one bad call that needs no device: every entry point refuses a NULL context"""
    from visual_odom_amd import build, _lib
    build.build()
    lib = _lib.load()
    assert lib.voflow_track(None, None, None, 64, 48, 64, None, 0, None, None, None) == _lib.VO_ERR_ARG
    assert lib.voflow_feature_tracking(None, None, None, 64, 48, 64, None, 0, None, None, None, None, None) == _lib.VO_ERR_ARG
    assert lib.voflow_batch_set_pairs(None, None, 1) == _lib.VO_ERR_ARG
    assert lib.voflow_batch_run(None) == _lib.VO_ERR_ARG
    assert lib.voflow_batch_get(None, 0, None, None, None, 0) == _lib.VO_ERR_ARG
