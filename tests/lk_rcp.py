"""The reciprocal programs (tests/host_check/rcp_check.hip on gfx950, rcp_host.cpp with g++): build and run, for
test_gpu_lk_level_setup.py."""
import os
import subprocess

import emu_build
from conftest import ROOT

SRC_DIR = os.path.join(ROOT, "tests", "host_check")
OPERANDS = 52 << 23     # every float of the exponents 2^-23 .. 2^28 (rcp_cases.h)
SAMPLES = 1 << 20


def build_host(out_dir):
    exe = os.path.join(out_dir, "rcp_host")
    emu_build.build(exe, os.path.join(SRC_DIR, "rcp_host.cpp"), emu_build.FLAGS + ["-O2"])
    return exe


def build_device(out_dir):
    """hipcc with the product's flags, as tests/lk_cols.py builds lk_cols_check"""
    from visual_odom_amd.build import FLAGS, HIPCC
    exe = os.path.join(out_dir, "rcp_check")
    subprocess.check_call([HIPCC] + [f for f in FLAGS if f != "-fPIC"] + ["-o", exe, os.path.join(SRC_DIR, "rcp_check.hip")])
    return exe


def run(exe, out_file):
    """one run under its own time limit: the words of its "OK" line; a non-zero exit, a signal or the time limit fails"""
    r = subprocess.run([exe, out_file], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, "%s exited with %d:\n%s\n%s" % (os.path.basename(exe), r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    word = r.stdout.split()
    assert word[0] == "OK", r.stdout
    assert os.path.getsize(out_file) == 4 * SAMPLES
    return [int(x) for x in word[1:]]
