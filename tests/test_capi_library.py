"""libvo_hip.so builds for gfx950 with hipcc (cross-compile, no GPU needed), loads, and exports every
symbol include/vo_hip.h declares.  No compute calls here."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built_lib():
    from visual_odom_amd import build, _lib
    build.build()
    return _lib.load()


def declared_symbols():
    hdr = open(os.path.join(ROOT, "include", "vo_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(vo_[a-z0-9_]+)\s*\(", hdr)))


def test_header_symbols_all_exported(built_lib):
    syms = declared_symbols()
    assert len(syms) >= 24
    for s in syms:
        assert hasattr(built_lib, s), "libvo_hip.so does not export %s" % s


def test_binding_list_matches_header():
    from visual_odom_amd import _lib
    assert sorted(_lib.EXPORTS) == declared_symbols()


def test_default_params_are_the_reference_literals(built_lib):
    from visual_odom_amd import _lib
    import ctypes as C
    p = _lib.VoParams()
    built_lib.vo_default_params(C.byref(p))
    assert (p.lk_max_level, p.lk_max_count, p.consistency_threshold, p.ransac_iterations) == (3, 30, 0, 500)
    assert p.lk_epsilon == 0.01 and p.lk_min_eig_threshold == 0.001     # feature.cpp:128,136
    assert p.ransac_reproj_error == 0.5                                  # visualOdometry.cpp:169
    import numpy as np
    assert p.ransac_confidence == float(np.float32(0.999))               # `float confidence = 0.999`


def test_no_gpu_means_loud_failure(built_lib):
    """without a HIP device the product must fail, never fall back to a CPU path"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from visual_odom_amd import _lib
    with pytest.raises(RuntimeError):
        _lib.Context(0, 640, 480, 1024, 1)


def test_product_does_not_import_oracle():
    pkg = os.path.join(ROOT, "visual_odom_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in txt.replace("never routes through the oracle", "") \
                    .replace("never a product fallback", ""), "%s mentions the oracle" % f


def test_detect_defaults_are_the_reference_literals(built_lib):
    from visual_odom_amd import _lib
    import ctypes as C
    p = _lib.VoDetectParams()
    built_lib.vo_default_detect_params(C.byref(p))
    # feature.cpp:43-45, visualOdometry.cpp:95,106-107
    assert (p.fast_threshold, p.fast_nonmax, p.redetect_below, p.bucket_size, p.features_per_bucket) == (20, 1, 2000, 0, 1)


def test_integrate_odometry_host_math(built_lib):
    """vo_integrate_odometry is host arithmetic inside libvo_hip (no device): gates and pose chaining of
    main.cpp:196-208 / utils.cpp:57-131 against the checker's restatement"""
    import numpy as np
    from visual_odom_amd import _lib
    from oracle import oracle as orc
    orc.build()
    rng = np.random.default_rng(0)
    pose_p = pose_o = np.eye(4)
    n_applied = 0
    for k in range(60):
        r = rng.normal(0, 0.03, 3)
        if k % 11 == 5:
            r[1] = 0.2            # yaw beyond the 0.1 rad gate
        t = rng.normal(0, 0.4, 3)
        if k % 7 == 3:
            t *= 0.01             # |t| below 0.05
        if k % 13 == 6:
            t *= 100              # |t| above 10
        R = orc.rodrigues(r)
        e_o = orc.rotation_matrix_to_euler(R)
        ok_o = False
        if abs(e_o[1]) < 0.1 and abs(e_o[0]) < 0.1 and abs(e_o[2]) < 0.1:
            pose_o, ok_o = orc.integrate_odometry_stereo(pose_o, R, t)
        pose_p, ok_p, e_p = _lib.integrate_odometry(pose_p, R, t)
        assert ok_p == ok_o and np.array_equal(e_p, e_o)
        assert np.abs(pose_p - pose_o).max() < 1e-12
        n_applied += ok_p
    assert 30 < n_applied < 58


def test_cpp_host_program_builds_and_fails_loudly_without_gpu(vo_run_binary, tmp_path):
    """the C++ mirror of main.cpp links against the C ABI; with no GPU it must exit non-zero, not fall back"""
    import subprocess
    import torch
    r = subprocess.run([vo_run_binary], capture_output=True, text=True)
    assert r.returncode == 1 and "usage" in r.stderr
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import numpy as np
    d = tmp_path / "seq"
    for cam in (0, 1):
        (d / ("image_%d" % cam)).mkdir(parents=True)
        for k in range(2):
            img = np.full((64, 96), 100 + k, np.uint8)
            with open(d / ("image_%d" % cam) / ("%06d.pgm" % k), "wb") as f:
                f.write(b"P5\n96 64\n255\n" + img.tobytes())
    r = subprocess.run([vo_run_binary, str(d), "300", "48", "32", "-100", "2", str(tmp_path / "p.txt")],
                       capture_output=True, text=True)
    assert r.returncode == 2 and "no HIP device" in r.stderr


def test_product_library_reads_no_environment_variable():
    """the fourteen getenv switches and the measured-slower kernel variants live in the developer build
    (python -m visual_odom_amd.build --dev -> libvo_hip_dev.so, -DVO_DEV_VARIANTS) only: libvo_hip.so does not even import
    getenv, and does not contain the two-features-per-wavefront LK kernel, the 128-register pose kernels or the 128 x 32 FAST tile"""
    import subprocess
    from visual_odom_amd import build
    so = build.build()
    und = subprocess.run(["nm", "-D", "--undefined-only", so], capture_output=True, text=True, check=True).stdout
    assert "getenv" not in und
    blob = open(so, "rb").read()
    for name in (b"lk_circular_pair_kernel", b"fast_tile_big_kernel"):
        assert name not in blob, name
    assert b"lk_circular_kernel" in blob and b"ransac_rest_kernel" in blob and b"pull_image_kernel" in blob
    # kernel symbols are mangled: epnp_kernel<4> / select_refine_kernel<4> = ...ILi4EE...
    # (epnp_kernel<WAVES, GWS>: GWS = true is the slim form of the round-4 experiment, developer build only)
    assert b"epnp_kernelILi4E" not in blob and b"select_refine_kernelILi4EE" not in blob and b"Lb1EE" not in blob
    assert b"epnp_kernelILi2ELb0EE" in blob and b"epnp_kernelILi1ELb0EE" in blob
    # the small-launch form of the pose solve is part of the product (pnp.hip, vo_svd_wide.h)
    for name in (b"epnp_prepare_kernel", b"svd12_wave_kernel", b"epnp_approx_kernel", b"epnp_select_kernel"):
        assert name in blob, name
    # the sources say the same: what only the developer build compiles lives in csrc/dev/, its hooks inside product sources go
    # through vo_dev_hooks.h, and the one guard left is the launch of the slim pose chain (two branches in pnp.hip -- a discarded
    # `if constexpr` would still instantiate the 128-register kernels into the product)
    csrc = os.path.join(os.path.dirname(build.__file__), "csrc")
    guards, getenvs = {}, []
    for f in sorted(os.listdir(csrc)):
        if f.endswith((".hip", ".h")) and f != "vo_dev_hooks.h":
            text = open(os.path.join(csrc, f)).read()
            if "VO_DEV_VARIANTS" in text:
                guards[f] = text.count("VO_DEV_VARIANTS")
            if "getenv" in text:
                getenvs.append(f)
    assert guards in ({}, {"pnp.hip": 1}, {"pnp.hip": 2}), guards
    assert not getenvs, getenvs
    for f in build.SOURCES:
        assert "/" not in f and os.path.exists(os.path.join(csrc, f)), f   # the product is built from csrc/*.hip alone


def test_product_library_exports_only_the_header():
    """the developer build adds entry points of its own (vo_dev_*: time stamps of the pose kernels); the product library's
    vo_* exports are exactly the functions include/vo_hip.h declares"""
    import subprocess
    from visual_odom_amd import build
    so = build.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln and ln.split()[-1].startswith("vo_")}
    assert exported == set(declared_symbols()), sorted(exported ^ set(declared_symbols()))


def test_frame_loop_host_logic_of_the_kept_pair():
    """host side of the kept pair (no device): NULL t0 images stay NULL on their way to the C ABI next to images that share
    a stride; StereoOdometry names the kept pair from its second frame on and hands all four images over again when the
    library says that it holds none (VO_ERR_STATE), without swallowing any other error"""
    import numpy as np
    from visual_odom_amd import _lib, odometry
    img = np.zeros((40, 64), np.uint8)
    pad = np.zeros((44, 80), np.uint8)
    arrs, stride = _lib._imgs_opt(None, None, pad[2:42, 8:72], pad[1:41, 3:67])
    assert arrs[0] is None and arrs[1] is None and stride == 80 and arrs[2].shape == (40, 64)
    arrs, stride = _lib._imgs_opt(None, img, img, pad[2:42, 8:72])           # (one NULL: the C ABI answers VO_ERR_ARG)
    assert arrs[0] is None and stride == 64 and all(a.flags["C_CONTIGUOUS"] for a in arrs[1:])
    assert _lib._pn(None) is None

    class FakeCtx:
        def __init__(self):
            self.calls, self.refuse, self.fail_code, self.gen = [], False, _lib.VO_ERR_STATE, 0

        def set_params(self, **kw):
            pass

        def kept_pair_id(self):
            return self.gen

        def detect_bucket(self, image, pts, ages, **kw):
            self.calls.append(("detect", image is None))
            if image is None and self.refuse:
                raise _lib.VoError(self.fail_code, "no kept pair")
            return np.zeros((8, 2), np.float32), np.zeros(8, np.int32)

        def track_frame(self, l0, r0, l1, r1, pts, P_l, P_r, tvec=None):
            self.calls.append(("track", l0 is None, r0 is None))
            self.gen += 1                                                  # every call leaves a new kept pair
            k = np.arange(6, dtype=np.int32)
            return dict(rc=0, l1=np.ones((6, 2), np.float32), keep_idx_circ=k, inliers=k, rvec=np.zeros(3),
                        tvec=np.array([0., 0., 0.5]), R=np.eye(3))

    P = np.hstack([np.eye(3), np.zeros((3, 1))]).astype(np.float32)
    fake = FakeCtx()
    vo = odometry.StereoOdometry(P, P, ctx=fake)
    for _ in range(3):
        vo.process(img, img)
    assert fake.calls == [("detect", False), ("track", False, False), ("detect", True), ("track", True, True)]
    fake.calls, fake.refuse = [], True                                        # somebody else used the context's images
    vo.process(img, img)
    assert fake.calls == [("detect", True), ("detect", False), ("track", False, False)]
    fake.calls, fake.refuse = [], False
    vo.process(img, img)
    assert fake.calls == [("detect", True), ("track", True, True)]             # (kept again after a four-image call)
    fake.refuse, fake.fail_code = True, _lib.VO_ERR_HIP
    with pytest.raises(_lib.VoError):
        vo.process(img, img)
    # a second user of the context (another loop, a direct call) leaves ANOTHER pair there -- no error from the
    # library, so the loop compares the pair's id with the one it saw after its own call and hands all four images over
    fake.refuse, fake.calls = False, []
    vo.process(img, img)                                                      # (four images after the failed call)
    fake.calls = []
    fake.gen += 1                                                             # somebody else's vo_track_frame
    vo.process(img, img)
    assert fake.calls == [("detect", False), ("track", False, False)]
    fake.calls = []
    vo.process(img, img)
    assert fake.calls == [("detect", True), ("track", True, True)]
    fake2 = FakeCtx()
    vo2 = odometry.StereoOdometry(P, P, ctx=fake2, keep_pair=False)
    for _ in range(3):
        vo2.process(img, img)
    assert all(c[1] is False for c in fake2.calls)


def test_adapter_is_shipped_source_and_the_only_copy():
    """adapters/feature_hip.{h,cpp} + USE_HIP.cmake are real files; the drop-in test build compiles THAT file
    (no second copy of circularMatching_hip anywhere), INTEGRATION.md points at the files instead of pasting them; the adapter
    compiling on its own against the reference's feature.h (C++11, -Wall -Werror) is a step of that build, which build() runs
    wherever the reference tree is there to compile against."""
    ad = os.path.join(ROOT, "adapters")
    for f in ("feature_hip.h", "feature_hip.cpp", "USE_HIP.cmake"):
        assert os.path.getsize(os.path.join(ad, f)) > 500, f
    hdr = open(os.path.join(ad, "feature_hip.h")).read()
    assert "__has_include(<opencv2/core.hpp>)" in hdr
    defs = []
    for dirpath, _, files in os.walk(ROOT):
        if any(s in dirpath for s in ("/.git", "/gpurun_out", "/_build", "/profiles")):
            continue
        for f in files:
            if f.endswith((".cpp", ".h", ".hip", ".md")):
                txt = open(os.path.join(dirpath, f), errors="replace").read()
                if "void circularMatching_hip(" in txt and "{" in txt.split("void circularMatching_hip(", 1)[1].split(";", 1)[0]:
                    defs.append(os.path.relpath(os.path.join(dirpath, f), ROOT))
    assert defs == ["adapters/feature_hip.cpp"], defs
    mk = open(os.path.join(ROOT, "oracle", "ref_dropin", "Makefile")).read()
    assert "adapters/feature_hip.cpp" in mk
    assert "-std=c++11 -Wall -Werror -fsyntax-only -I$(ROOT)/oracle/ref_shim -I$(REF)/src -I$(ROOT)/include" in mk
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "adapters/feature_hip.cpp" in integ and "adapters/USE_HIP.cmake" in integ
