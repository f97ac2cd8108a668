"""tests/host_check/device_check.hip without a GPU: the program the GPU suite runs once on the MI355X
(tests/test_gpu_device_units.py), built here with the same hipcc command and started with --host, where it runs the host side
of the same entry points over the same input files.  Its outputs must equal the g++ build's (host_check.cpp: hc_case) bit for
bit: that pins the file layout, the decoding of the operations and the agreement of clang's host code with g++'s, so that on
the GPU box a difference can only come from the device.  Also here: the properties of the vectors themselves that the GPU
test relies on."""
import os
import subprocess

import numpy as np
import pytest

import device_vectors as dv
from conftest import vp

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc on this machine")

HOST_OPS = [n for n in dv.OUT_TYPES if n not in dv.DEVICE_ONLY]


@pytest.fixture(scope="module")
def host_run(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("device_check_host"))
    exe, _ = dv.build_device_check(d)
    ins = dv.device_check_inputs()
    dv.write_inputs(d, ins)     # (the device-only operations' files too: --host must leave them alone)
    r = subprocess.run([exe, "--host", d], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    done = r.stdout.split()
    assert done[0] == "OK" and sorted(done[1:]) == sorted(HOST_OPS), r.stdout
    assert not any(os.path.exists(os.path.join(d, n + ".out")) for n in dv.DEVICE_ONLY)
    return ins, dv.read_outputs(d, ins, HOST_OPS), exe


@pytest.mark.parametrize("name", HOST_OPS)
def test_host_mode_equals_the_gpp_build(host_run, host_check, name):
    ins, outs, _ = host_run
    want = dv.host_reference(host_check, ins, name)
    got = outs[name]
    if name in ("math_cos", "math_sin"):    # NaN / +-inf: the platform's function answers; by class only
        nf = len(dv.TRIG_NONFINITE)
        assert np.isnan(got[-nf:]).all() and np.isnan(want[-nf:]).all()
        got, want = got[:-nf], want[:-nf]
    msg = dv.first_difference(name, got, want, ins[name][:len(got)])
    assert msg is None, msg


def test_generic_entry_point_equals_the_named_exports(host_run, host_check):
    """hc_case runs the same header code as the exports the CPU tests have always used"""
    ins, outs, _ = host_run
    top, bot, w = dv.bilinear_operands()
    got = np.zeros((len(top), 7), np.int16)
    host_check.hc_bilinear7_u8(vp(top), vp(bot), vp(w), len(top), vp(got))
    assert np.array_equal(got, outs["lk_bilinear7_u8"]) and np.array_equal(got, outs["lk_blend7"])
    A, b = dv.solve6_systems()
    x = np.zeros(6)
    host_check.hc_solve6(vp(A[0]), vp(b[0]), vp(x))
    assert np.array_equal(x.view(np.uint64), outs["solve6"][0].view(np.uint64))
    x = np.array(dv.CBRT_EDGES + [2.5])
    y = np.zeros_like(x)
    host_check.hc_math(0, vp(x), len(x), vp(y))
    n = len(dv.CBRT_EDGES)
    assert np.array_equal(y[:n].view(np.uint64), outs["math_cbrt"][-n:, 0].view(np.uint64))


def test_a_malformed_input_stops_the_program(host_run, tmp_path):
    exe = host_run[2]
    np.zeros(5, np.uint8).tofile(str(tmp_path / "math_cbrt.in"))      # no multiple of the 8-byte record
    r = subprocess.run([exe, "--host", str(tmp_path)], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and r.stdout.startswith("FAIL:")


def test_row_sum_sets_tell_summation_orders_apart():
    """the GPU test of row_ordered_sum compares with the serial left-to-right sum: for EVERY set of terms the reversed, the
    pairwise and the sorted sum give other bits, so a chain in another order cannot pass; lanes N .. 15 hold NaN; every DPP row
    has a set of its own"""
    sets = dv.row_sum_sets()
    v = sets.reshape(len(sets), 4, 4, 16)
    assert np.isnan(v[:, :2, :, 6:]).all() and np.isnan(v[:, 2:, :, 12:]).all()
    for terms in dv.row_sum_terms(sets):
        assert np.isfinite(terms).all()
        s = dv.serial_sum(terms)
        for other in dv.other_order_sums(terms):
            assert (other.view(np.uint64) != s.view(np.uint64)).all()
        mag = np.log2(np.abs(terms))
        assert (mag.max(-1) - mag.min(-1)).max() >= 40 and (terms > 0).any() and (terms < 0).any()
        assert len(np.unique(s)) > 0.9 * s.size          # a different sum in (nearly) every row of every case


def test_the_bit_exact_trig_sets_stay_below_the_hand_over():
    x = dv.trig_large_args()
    assert np.abs(x).max() < dv.TRIG_BOUND and np.abs(x).max() > dv.TRIG_BOUND - 1e-6
    k = np.rint(np.abs(x) / (np.pi / 2))
    near = np.abs(np.abs(x) - k * (np.pi / 2)) < 2e-9
    assert near.sum() >= 512 and k[near].max() == 2 ** 19 - 1
    for name in ("math_cos", "math_sin"):
        a = dv.device_check_inputs.__globals__["cos_args" if name == "math_cos" else "sin_args"]()
        assert np.abs(a).max() < dv.TRIG_BOUND
