"""Build libvo_hip.so (hand-written HIP for gfx950) in-tree with hipcc.

    python -m visual_odom_amd.build [--force] [--dev]

The product library is built from SOURCES (csrc/*.hip) and reads no environment variable, neither when it is built nor when it runs.

--dev additionally builds libvo_hip_dev.so from DEV_SOURCES with -DVO_DEV_VARIANTS: the same library plus what csrc/dev/ holds.
A wrapper there (dev/lk_dev.hip, dev/pyramid_dev.hip, dev/fast_dev.hip, dev/pnp_dev.hip) is compiled INSTEAD of the product file
it includes and adds the kernel variants that were built, measured and lost (two-features-per-wavefront LK, the round-3
three-kernel pyramid chain, 128 x 32 FAST tile, ordinary-store Scharr) with the environment switches that select them
(VO_LK_PAIR, VO_PYR_FUSED, VO_PYR_LDS, VO_PYR_STORE, VO_SCHARR_NT, VO_FAST_TILE); dev/capi_dev.hip adds the vo_dev_* entry
points.  -DVO_DEV_VARIANTS also turns on the hooks of csrc/vo_dev_hooks.h inside the product sources (tuning switches such as
VO_SERIAL_POSE, time stamps in the pose kernels) and the 128-register pose kernels (vo_set_schedule pose_waves = 4).  The
environment variable VO_LK_ATTRS (register caps of the LK kernel, tools/gpu_lk_sweep.sh) reaches the developer build only.
tools/ uses that library (VO_HIP_LIB=.../libvo_hip_dev.so).

Flags that matter for parity: -ffp-contract=off (no FMA contraction: the f32 2x2 LK solve and the
f64 pose math must round like the CPU path) and correctly rounded f32 divide / sqrt.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(CSRC, "_obj")
SO = os.path.join(HERE, "libvo_hip.so")
SOURCES = ["pyramid.hip", "fast.hip", "lk.hip", "post.hip", "pnp.hip", "essential.hip", "seq.hip", "ingest_fmt.hip", "rectify.hip", "capi.hip", "capi_run.hip",
           "capi_sched.hip", "capi_seq.hip", "capi_dropin.hip", "capi_flow.hip", "corners.hip", "capi_corners.hip", "capi_corners_mask.hip",
           "capi_corners_response.hip", "capi_detector.hip", "capi_topup.hip", "capi_fast_mask.hip"]
# the developer build: a wrapper in place of the product file it includes, and the entry points of its own
DEV_WRAPPERS = {"pyramid.hip": "dev/pyramid_dev.hip", "fast.hip": "dev/fast_dev.hip", "lk.hip": "dev/lk_dev.hip", "pnp.hip": "dev/pnp_dev.hip"}
DEV_SOURCES = [DEV_WRAPPERS.get(s, s) for s in SOURCES] + ["dev/capi_dev.hip"]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
         "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-fast-math", "-Wall", "-Wno-unused-function"]


def _newer(target, deps):
    return os.path.exists(target) and all(os.path.getmtime(target) >= os.path.getmtime(d) for d in deps)


def build(force=False, verbose=False, dev=False):
    obj_dir = OBJ + ("_dev" if dev else "")
    so = SO.replace("libvo_hip.so", "libvo_hip_dev.so") if dev else SO
    os.makedirs(obj_dir, exist_ok=True)
    flags = list(FLAGS)
    if dev:
        flags.append("-DVO_DEV_VARIANTS")
        if os.environ.get("VO_LK_ATTRS"):  # developer A/B of the LK kernel's register caps
            flags.append("-DVO_LK_ATTRS=" + os.environ["VO_LK_ATTRS"])
    headers = [os.path.join(d, f) for d in (CSRC, os.path.join(CSRC, "dev")) for f in os.listdir(d) if f.endswith(".h")]
    headers += [os.path.join(HERE, "..", "include", f) for f in ("vo_hip.h", "vo_flow.h", "vo_flow_win.h", "vo_flow_flags.h", "vo_corners.h", "vo_corners_mask.h",
                                                          "vo_corners_response.h", "vo_detector.h", "vo_topup.h", "vo_fast_mask.h")]
    wrapped = {w: s for s, w in DEV_WRAPPERS.items()}
    objs, jobs = [], []
    for s in (DEV_SOURCES if dev else SOURCES):
        src = os.path.join(CSRC, s)
        obj = os.path.join(obj_dir, os.path.basename(s).replace(".hip", ".o"))
        objs.append(obj)
        deps = [src] + headers + ([os.path.join(CSRC, wrapped[s])] if s in wrapped else [])
        if force or not _newer(obj, deps):
            jobs.append([HIPCC] + flags + ["-c", src, "-o", obj])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed:\n%s\n%s" % (" ".join(cmd), r.stderr[-8000:]))
        return r.stderr

    with ThreadPoolExecutor(max_workers=5) as ex:
        for msg in ex.map(run, jobs):
            if verbose and msg.strip():
                print(msg)
    if force or jobs or not _newer(so, objs):
        run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", so] + objs)
    return so


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
    if "--dev" in sys.argv:
        print(build(force="--force" in sys.argv, verbose=True, dev=True))
