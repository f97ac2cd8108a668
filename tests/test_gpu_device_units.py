"""The unit vectors of the device-math headers run ON gfx950 (tests/host_check/device_check.hip: one small program, compiled
with the product's flags, started ONCE) -- the device branches of every `#if defined(__HIP_DEVICE_COMPILE__)` that the CPU
suite can only compile the other side of: v_perm_b32 / v_dot2 / v_pk_* / v_cvt_pk_i16_i32 / v_alignbyte behind the wrappers
of vo_isa.h and vo_lkmath.h, the v_mov_b64_dpp row_newbcast + v_add_f64 chains of vo_svd_wide.h under a partly masked EXEC, and the f64 pose math
(vo_math.h, vo_linalg.h, vo_epnp.h, vo_p3p.h, vo_fivept.h, vo_tri.h) as gfx950 code.

Three kinds of checks, all with margin ZERO unless said otherwise:
  * device == the g++ build of the same entry point (host_check.cpp: hc_case), compared as unsigned integers, NaN payloads
    included.  This is the design the headers state (IEEE operations only, no contraction, correctly rounded divide and sqrt),
    not a measured tolerance;
  * wide == serial, both on the device: the row-cooperative SVD, the wavefront 6 x 6 solve in both launch shapes, the
    four-kernel EPnP; the ordered row sums against the serial left-to-right f64 sum formed by numpy;
  * against references that do not share the code: numpy longdouble (1 ulp, the bound tests/test_vo_math.py holds the host
    to), the plain int64 DESCALE formulas, numpy restatements of every instruction wrapper, SVD / solve identities.
The same vectors (tests/device_vectors.py) feed the CPU tests; tests/test_device_check_host_mode.py runs this program's host
side without a GPU."""
import os
import subprocess
import time

import numpy as np
import pytest

import device_vectors as dv

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(tmp_path_factory):
    """build once, write every input, ONE run under its own time limit, every output.  A non-zero exit, a signal or the time
    limit fails the fixture: nothing starts the program a second time."""
    d = str(tmp_path_factory.mktemp("device_check"))
    exe, t_build = dv.build_device_check(d)
    ins = dv.device_check_inputs()
    dv.write_inputs(d, ins)
    t0 = time.time()
    r = subprocess.run([exe, d], capture_output=True, text=True, timeout=120)
    t_run = time.time() - t0
    assert r.returncode == 0, "device_check exited with %d:\n%s\n%s" % (r.returncode, r.stdout[-4000:], r.stderr[-4000:])
    done = r.stdout.split()
    assert done[0] == "OK" and sorted(done[1:]) == sorted(ins), r.stdout
    outs = dv.read_outputs(d, ins, ins.keys())
    print("device_check: build %.1f s, run %.2f s; cases: %s" % (t_build, t_run, ", ".join("%s %d" % (k, len(v)) for k, v in ins.items())))
    return ins, outs


def same_bits(name, got, want, operands=None):
    msg = dv.first_difference(name, got, want, operands)
    assert msg is None, msg


def equals_host(dev, host_check, name, rows=slice(None)):
    ins, outs = dev
    want = dv.host_reference(host_check, ins, name)
    msg = dv.first_difference(name, outs[name][rows], want[rows], np.ascontiguousarray(ins[name])[rows])
    assert msg is None, "device != host build: " + msg
    return outs[name]


def _ulps(y, ref):
    return np.abs(y.astype(np.longdouble) - ref) / np.spacing(np.abs(ref.astype(np.float64))).astype(np.longdouble)


def test_vo_math_on_the_device(dev, host_check):
    """vo_cbrt / vo_acos / vo_cos / vo_sin / vo_lm_lambda: the host build's bits, and within one ulp of numpy's extended
    precision.  cos / sin: up to the hand-over bound 823549.6 (beyond it the platform's function answers and the header says
    it is not bit-portable: out of scope), the last three arguments (NaN, +-inf) by class only."""
    ins, outs = dev
    nf = len(dv.TRIG_NONFINITE)
    for name, fn, rows in (("math_cbrt", np.cbrt, slice(None)), ("math_acos", np.arccos, slice(None)), ("math_cos", np.cos, slice(0, -nf)),
                           ("math_sin", np.sin, slice(0, -nf))):
        y = equals_host(dev, host_check, name, rows)[rows, 0]
        x = ins[name][rows]
        assert name not in ("math_cos", "math_sin") or np.abs(x).max() < dv.TRIG_BOUND
        with np.errstate(invalid="ignore"):
            err = _ulps(y, fn(x.astype(np.longdouble)))
        err = err[np.isfinite(err)]
        print("%s: %d arguments, worst %.3f ulp" % (name, len(x), float(err.max())))
        assert len(err) > 0.99 * len(x) and float(err.max()) < 1.0, (name, float(err.max()))
    for name in ("math_cos", "math_sin"):
        assert np.isnan(outs[name][-nf:, 0]).all()      # NaN stays NaN, cos / sin of an infinity is NaN
    e = outs["math_cbrt"][-len(dv.CBRT_EDGES):, 0]
    assert e[0] == 0 and np.isnan(e[1]) and np.isinf(e[2]) and np.isnan(e[3]) and e[4] == 2.0 and e[5] == 3.0
    e = outs["math_acos"][-len(dv.ACOS_EDGES):, 0]
    assert e[0] == 0 and e[1] == np.pi and np.all(np.isnan(e[2:]))
    equals_host(dev, host_check, "math_lambda")
    import math
    k = np.clip(ins["math_lambda"], -16, 16)
    assert np.array_equal(outs["math_lambda"][:, 0], np.array([math.exp(int(i) * math.log(10.0)) for i in k]))


POSE_OPS = ["epnp5", "p3p4", "p3p_deg4", "rodrigues_v2m", "rodrigues_m2v", "triangulate", "five_point", "sampson", "decompose",
            "cheirality", "solve6", "svd12"]


@pytest.mark.parametrize("name", POSE_OPS)
def test_pose_headers_on_the_device(dev, host_check, name):
    """one thread per case, the routine as the pose kernels inline it: the host build's bits"""
    # five_point's last case (no motion at all) has no finite model: its E come out of 0 / 0.  IEEE 754 leaves the sign of a NaN
    # that an invalid operation CREATES to the implementation, and the two differ: gfx950 makes 0x7ff8000000000000, x86's SSE
    # 0xfff8000000000000 (seen on the MI355X: case 192, output 1).  No header can hold that, so this one case is compared bit
    # for bit only where the host's value is no NaN, and by class where it is; every other case of every operation bit for bit.
    rows = slice(0, -1) if name == "five_point" else slice(None)
    out = equals_host(dev, host_check, name, rows)
    if name == "five_point":
        got, want = out[-1], dv.host_reference(host_check, dev[0], name)[-1]
        nan = np.isnan(want)
        assert nan.any() and want[0] > 0 and np.isnan(got[nan]).all()
        same_bits("five_point, the case without motion, outside its NaN", got[~nan], want[~nan])
    # the sets exercise the routines: solutions exist, both answers of a predicate occur
    if name in ("p3p4", "p3p_deg4", "five_point"):
        assert (out[:, 0] > 0).mean() > 0.5 and np.isfinite(out[rows]).all()
    if name == "cheirality":
        assert 0.2 < out.mean() < 0.8
    if name == "rodrigues_m2v":   # and the round trip returns the vector (|r| < pi)
        r = dev[0]["rodrigues_v2m"][:1000]
        assert np.abs(out[:1000] - r).max() <= 1e-14


def test_row_cooperative_svd12_on_the_device(dev, host_check):
    """svd12_wave_kernel's body (128 threads per matrix in LDS: the DPP chains, two wavefronts, workgroup barriers) against the
    one-lane jacobi_svd<12, 12, false> ON THE DEVICE, bit for bit, and both against the host build; on the first matrix the
    existing SVD identities"""
    ins, outs = dev
    serial = equals_host(dev, host_check, "svd12")[:, :144]
    assert np.isfinite(serial).all()
    same_bits("svd12_wide (wide != serial, both on the device)", outs["svd12_wide"], np.ascontiguousarray(serial), ins["svd12_wide"])
    mats = ins["svd12_wide"].reshape(-1, 12, 12)
    U = outs["svd12_wide"][0].reshape(12, 12)
    assert np.allclose(U @ U.T, np.eye(12), atol=1e-12)
    assert np.abs(mats[0] @ U[10:].T).max() < 1e-6 * np.abs(mats[0]).max()


def test_wavefront_6x6_solve_on_the_device(dev, host_check):
    """jacobi6v_wave_sweeps + jacobi_finish + svd_backsubst, one wavefront per workgroup and four per workgroup without a
    workgroup barrier (select_refine_kernel's shape; 43 systems: the last workgroup has an idle wavefront), against
    solve_svd<6, 6> on the device and on the host"""
    ins, outs = dev
    serial = equals_host(dev, host_check, "solve6")
    assert np.isfinite(serial).all()
    for shape in ("solve6_wave1", "solve6_wave4"):
        same_bits(shape + " (wavefront != solve_svd, both on the device)", outs[shape], serial, ins[shape])
    A, b = ins["solve6"][:, :36].reshape(-1, 6, 6), ins["solve6"][:, 36:]
    x = outs["solve6_wave4"]
    assert np.allclose(A[0] @ x[0], b[0], rtol=1e-8)
    # every full-rank system: a backward-stable solve leaves |A x - b| <= c eps (|A| |x| + |b|) whatever the condition number;
    # 1e-8 is c = 4.5e7 units of eps = 2.2e-16
    for q in range(41):
        res = np.abs(A[q] @ x[q] - b[q]).max()
        assert res <= 1e-8 * (np.abs(A[q]).sum(1).max() * np.abs(x[q]).max() + np.abs(b[q]).max()), q


def test_four_kernel_epnp_on_the_device(dev, host_check):
    """epnp5_prepare<64> (LDS) | wide SVD | epnp5_L_rho<1> + epnp5_approx<1, a> | epnp5_select as four kernels, against
    epnp5_solve on the device, against the host build (which tests/test_device_math_on_host.py holds to the oracle)"""
    ins, outs = dev
    mono = equals_host(dev, host_check, "epnp5")
    assert np.isfinite(mono).all()
    same_bits("epnp_split (four kernels != epnp5_solve, both on the device)", outs["epnp_split"], mono, ins["epnp_split"])


def test_ordered_row_sums_on_the_device(dev):
    """row_ordered_sum<6 / 12> and row_ordered_sum_x2<6 / 12> called directly, one value per lane: every lane of a DPP row holds
    ((0 + x_0) + x_1) + ... + x_{N-1} of ITS row -- terms whose sum depends on the order (tests/test_device_check_host_mode.py
    checks that reversed, pairwise and sorted sums all differ), NaN in lanes N .. 15 -- with all four rows active, and with
    rows 0 and 2 switched off (they keep the sentinel)"""
    ins, outs = dev
    sets = ins["row_sums"].reshape(-1, 4, 64)
    x6, y6, x12, y12 = (dv.serial_sum(v) for v in dv.row_sum_terms(sets))      # (n, 4 rows)
    got = outs["row_sums"].reshape(-1, 2, 6, 4, 16)                             # case, mode, output, DPP row, lane
    want = np.empty_like(got)
    for k, s in enumerate((x6, x12, x6, y6, x12, y12)):
        want[:, 0, k] = s[:, :, None]
    for k, s in enumerate((y6, y12, y6, x6, y12, x12)):                          # the masked pass has the operands swapped
        want[:, 1, k] = s[:, :, None]
    want[:, 1, :, 0::2] = dv.ROW_SUMS_SENTINEL
    assert np.isfinite(want).all()
    names = ["sum<6>", "sum<12>", "sum_x2<6>.x", "sum_x2<6>.y", "sum_x2<12>.x", "sum_x2<12>.y"]
    bad = np.argwhere(got.view(np.uint64) != want.view(np.uint64))
    if len(bad):
        c, m, k, r, l = bad[0]
        raise AssertionError("row_sums: %d values differ; first: case %d, %s, row_ordered_%s, DPP row %d, lane %d: got %s want %s"
                             % (len(bad), c, ["all rows active", "rows 1 and 3 active"][m], names[k], r, l,
                                float(got[c, m, k, r, l]).hex(), float(want[c, m, k, r, l]).hex()))


def _lanes(v, signed=False):
    v = v.astype(np.int64)
    lo, hi = v & 0xffff, v >> 16
    if signed:
        lo, hi = lo - ((lo & 0x8000) << 1), hi - ((hi & 0x8000) << 1)
    return lo, hi


def _pk(lo, hi):
    return ((lo & 0xffff) | ((hi & 0xffff) << 16)).astype(np.uint32)


def _raw_restatement(name, a, b, c):
    """the instruction's definition in numpy (int64 arithmetic, truncated at the end)"""
    a, b, c = (np.ascontiguousarray(v) for v in (a, b, c))
    A, B, C_ = a.astype(np.int64), b.astype(np.int64), c.astype(np.int64)
    m32 = 0xffffffff
    if name == "perm_b32":
        data = np.concatenate([b.reshape(-1, 1).view(np.uint8), a.reshape(-1, 1).view(np.uint8)], 1)   # bytes 0 .. 3 lo, 4 .. 7 hi
        sel = c.reshape(-1, 1).view(np.uint8)
        out = np.where(sel <= 7, np.take_along_axis(data, np.minimum(sel, 7).astype(np.int64), 1), 0).astype(np.uint8)
        return np.ascontiguousarray(out).view(np.uint32)[:, 0]
    if name == "udot2":
        (al, ah), (bl, bh) = _lanes(a), _lanes(b)
        return ((al * bl + ah * bh + C_) & m32).astype(np.uint32)
    if name in ("sdot2", "sdot2_first"):
        (al, ah), (bl, bh) = _lanes(a, True), _lanes(b, True)
        acc = C_ - ((C_ & 0x80000000) << 1)
        s = al * bl + ah * bh + acc
        assert np.abs(s).max() < 2 ** 31                      # inside the documented ranges the clamp never acts
        return (s & m32).astype(np.uint32)
    (al, ah), (bl, bh), (cl, ch) = _lanes(a), _lanes(b), _lanes(c)
    if name == "pk_sub_i16":
        return _pk(al - bl, ah - bh)
    if name == "pk_lshr1_u16":
        return _pk(al >> 1, ah >> 1)
    if name == "udot4":
        return ((sum(((A >> s) & 0xff) * ((B >> s) & 0xff) for s in (0, 8, 16, 24)) + C_) & m32).astype(np.uint32)
    if name == "pk_add_u16":
        return _pk(al + bl, ah + bh)
    if name == "pk_subsat_u16":
        return _pk(np.maximum(al - bl, 0), np.maximum(ah - bh, 0))
    if name == "pk_min_u16":
        return _pk(np.minimum(al, bl), np.minimum(ah, bh))
    if name == "pk_mad_u16":
        return _pk(al * bl + cl, ah * bl + ch)               # k = the low 16 bits of b, for both lanes
    if name == "alignbyte":
        return ((((a.astype(np.uint64) << np.uint64(32)) | b.astype(np.uint64)) >> (c.astype(np.uint64) * np.uint64(8))) & np.uint64(m32)).astype(np.uint32)
    if name == "pack_w":
        return _pk(A, B)                                      # |w| <= 2^14: int16 holds it, no saturation
    if name == "pk_absdiff_i16":
        (al, ah), (bl, bh) = _lanes(a, True), _lanes(b, True)
        # 2^14 - (-2^14) = 2^15 is the one difference of the operands beyond int16; its lane reads 0x8000 either way: as the
        # u16 the err epilogue's v_dot2_u32_u16 takes, the result is |a - b| up to and including 2^15
        assert max(np.abs(al - bl).max(), np.abs(ah - bh).max()) <= 2 ** 15
        return _pk(np.abs(al - bl), np.abs(ah - bh))
    raise KeyError(name)


@pytest.mark.parametrize("name", dv.LK_RAW)
def test_lk_instruction_wrappers_on_the_device(dev, host_check, name):
    """the CDNA4 instruction behind each wrapper of vo_isa.h (and pack_w of vo_lkmath.h) against the wrapper's host text (plain C) and against a numpy
    restatement, on 2^20 random operand triples and the edges (tests/device_vectors.py: lk_raw_operands)"""
    ins, outs = dev
    op = ins["lk_" + name]
    assert len(op) > dv.N_RAW
    got = equals_host(dev, host_check, "lk_" + name)
    same_bits("lk_" + name + " (device != numpy restatement)", got[:, 0], _raw_restatement(name, op[:, 0], op[:, 1], op[:, 2]), op)
    if name == "sdot2_first":                                  # the clamped form and the plain one: same operands, same results
        assert np.array_equal(ins["lk_sdot2"], op)
        same_bits("lk_sdot2_first != lk_sdot2", got, outs["lk_sdot2"])


def test_lk_composites_on_the_device(dev, host_check):
    """bilinear7_u8, blend7(lift7, lift7), bilinear7_deriv, the pk_sub_i16 + sdot2 chain and scharr4_packed: the host build's
    bits and the plain int64 DESCALE formulas of tests/test_device_math_on_host.py"""
    ins, outs = dev
    top, bot, w = dv.bilinear_operands()
    ref = dv.bilinear_reference(top, bot, w)
    for name in ("lk_bilinear7_u8", "lk_blend7"):
        got = equals_host(dev, host_check, name)
        assert np.array_equal(got, ref), name
    assert ref.max() == 8160 and ref[8:12].min() >= 0
    dx, dy, packed, w = dv.deriv_operands()
    got = equals_host(dev, host_check, "lk_bilinear7_deriv")
    assert np.array_equal(got[:, :7], dv.deriv_reference(dx, w)) and np.array_equal(got[:, 7:], dv.deriv_reference(dy, w))
    val, I, ix = dv.diff_dot_operands()
    got = equals_host(dev, host_check, "lk_diff_dot")
    ref = ((val.astype(np.int64) - I) * ix).sum(1)
    assert np.array_equal(got[:, 0], ref) and abs(ref).max() < 2**28
    got = equals_host(dev, host_check, "lk_scharr4")[:, 0]
    p = ins["lk_scharr4"].astype(np.int64)
    gx = (p[:, 2] + p[:, 7]) * 3 + p[:, 4] * 10 - (p[:, 0] + p[:, 5]) * 3 - p[:, 3] * 10
    gy = (p[:, 5] + p[:, 7]) * 3 + p[:, 6] * 10 - (p[:, 0] + p[:, 2]) * 3 - p[:, 1] * 10
    assert np.array_equal(got, _pk(4 * gx, 4 * gy)) and (4 * gx).max() == 16320 and (4 * gy).min() == -16320


def test_fast_compass_pair_on_the_device(dev):
    """fast_compass_pair (v_pk_add_u16, v_pk_sub_u16 clamp, v_pk_min_u16) against the scalar fast_compass_candidate over the
    sweep of ke_fast_compass_pair_check, generated and compared on the device: no disagreement, every comparison made"""
    raw = dev[1]["fast_pair"]
    bad, done = raw[:16].view(np.uint64)
    n_centres = len([v for v in _centres()])
    assert done == 8 * n_centres * 9 ** 4 * 2, done
    tuples = raw[16:].view(np.uint32).reshape(-1, 8)
    assert bad == 0, "fast_pair: %d disagreements; first {v, c0, c4, c8, c12, t2, result, wanted}: %s" % (
        bad, [" ".join("%#x" % x for x in t) for t in tuples[:min(int(bad), len(tuples))]])


def _centres():
    v0 = 0
    while v0 < 256:
        yield v0
        v0 += 1 if (v0 < 24 or v0 > 230) else 5
