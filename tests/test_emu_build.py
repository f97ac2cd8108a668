"""tests/emu_build.py: a target is rebuilt exactly when what the compiler read for it says so, and the real harnesses' dependency
files name the headers a hand-written list used to miss."""
import os
import subprocess

import pytest

import emu_build


def test_rebuilds_when_and_only_when_a_dependency_says_so(tmp_path):
    d = str(tmp_path)
    hdr, so = os.path.join(d, "answer.h"), os.path.join(d, "libanswer.so")
    with open(hdr, "w") as f:
        f.write("#define ANSWER 41\n")
    with open(os.path.join(d, "answer.cpp"), "w") as f:
        f.write('#include "answer.h"\nextern "C" int answer()\n{\n    return ANSWER;\n}\n')
    load = lambda: emu_build.shared("answer", out_dir=d, src_dir=d)
    ident = lambda: (os.stat(so).st_mtime_ns, os.stat(so).st_ino)
    assert load().answer() == 41
    first = ident()
    assert load().answer() == 41 and ident() == first          # up to date: not rebuilt
    os.utime(hdr, ns=(first[0] + 10 ** 9,) * 2)                  # the header is newer than the library
    load()
    second = ident()
    assert second != first
    os.utime(hdr, ns=(first[0],) * 2)
    load()
    assert ident() == second
    os.remove(so + ".d")                                         # no record of what was read
    load()
    third = ident()
    assert third != second and os.path.exists(so + ".d")
    load = lambda: emu_build.shared("answer", ["-DUNUSED"], out_dir=d, src_dir=d)   # another command line
    load()
    fourth = ident()
    assert fourth != third
    load()
    assert ident() == fourth
    os.remove(hdr)                                               # the compiler's error, not the old library
    with pytest.raises(subprocess.CalledProcessError):
        load()


def test_dependency_files_of_the_lk_harnesses_name_what_lk_hip_includes():
    import flow_emu
    import lk_chain_cases
    flow_emu.load()
    lk_chain_cases.emu_lib()
    for lib in ("libflow_emu.so", "libchain_emu.so"):
        with open(os.path.join(emu_build.OUT_DIR, lib + ".d")) as f:
            deps = {os.path.basename(p) for p in f.read().split()}
        assert {"vo_lkqueue.h", "vo_dev_hooks.h", "lk.hip", "emu_pyramid.h", "hip_emu.h"} <= deps, (lib, sorted(deps))
