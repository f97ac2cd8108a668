"""The unit-vector programs of the vertical-pair samplers (tests/host_check/lk_cols_cases.h): build and run, shared by
test_lk_cols_on_host.py (g++, the host text of vo_lkmath.h) and test_gpu_lk_cols.py (the same vectors on gfx950)."""
import os
import subprocess

import emu_build
from conftest import ROOT

SRC_DIR = os.path.join(ROOT, "tests", "host_check")
RECORD = 48   # bytes of a ColsOut: val[4], ix[4], iy[4]


def build_host(out_dir):
    exe = os.path.join(out_dir, "lk_cols_host")
    emu_build.build(exe, os.path.join(SRC_DIR, "lk_cols_host.cpp"), emu_build.FLAGS + ["-O2"])
    return exe


def build_device(out_dir):
    """hipcc with the product's flags, as tests/device_vectors.py builds device_check"""
    from visual_odom_amd.build import FLAGS, HIPCC
    exe = os.path.join(out_dir, "lk_cols_check")
    subprocess.check_call([HIPCC] + [f for f in FLAGS if f != "-fPIC"] + ["-o", exe, os.path.join(SRC_DIR, "lk_cols_check.hip")])
    return exe


def run(exe, out_file):
    """one run under its own time limit: (cases, cases with iw11 < 0) of its "OK" line; anything else fails"""
    r = subprocess.run([exe, out_file], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, "%s exited with %d:\n%s\n%s" % (os.path.basename(exe), r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    word = r.stdout.split()
    assert word[0] == "OK" and len(word) == 3, r.stdout
    n, n_neg = int(word[1]), int(word[2])
    assert os.path.getsize(out_file) == n * RECORD
    return n, n_neg
