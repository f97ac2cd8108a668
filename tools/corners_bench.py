"""What the Shi-Tomasi detector (include/vo_corners.h) costs on the MI355X.

  throughput  vocorn_batch_run over `--images` resident 1241 x 376 images (rendered KITTI-shaped frames, `--frames` distinct ones
              repeated) at the reference's parameters (5000, 0.01, 5.0): ms per run = wall time of `--runs` back-to-back runs up
              to the synchronise / runs, `--repeats` times after a warm-up; the spread over the repeats is the noise figure.
              Beside it on the same table in the same process, alternating within a repeat: vo_batch_run(VO_STAGE_DETECT) -- the
              FAST detect + bucketing stage of the same tree on the same left images -- as context.
  latency     one synchronous vocorn_detect (upload, three kernels, two small copies back) next to vo_fast_detect: median and
              min of `--calls` calls each.
  baseline    tests/host_check/corners_ref.c, single-threaded on this host's CPU, per image.
  kernels     per-kernel times come from the profiler, in a run of its own:
                  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/corners_bench.py --runs 3 --repeats 1 --calls 0 --no-cpu
              (kernel names: corn_map_kernel, corn_cand_kernel, corn_select_kernel).
  rounds      the suppression's round count is a property of the image; it is reported from the CPU emulator of the same kernel
              source on the first frame (--rounds).

    python tools/corners_bench.py [--images 256] [--frames 8] [--runs 10] [--repeats 5] [--calls 100] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H = 1241, 376


def stats(t):
    t = np.asarray(t, np.float64)
    return dict(median_ms=float(np.median(t)), min_ms=float(t.min()), max_ms=float(t.max()), n=int(len(t)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--rounds", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    from visual_odom_amd import _lib, synth
    world = synth.StereoWorld(seed=20260925)
    lefts, _, _, _ = world.render_sequence(args.frames)
    B = args.images
    out = dict(images=B, w=W, h=H, params=dict(max_corners=5000, quality_level=0.01, min_distance=5.0))

    ctx = _lib.Context(0, W, H, 4096, B)
    ctx.batch_configure(4 * B, W, H, B)
    for f in range(B):   # the left image of frame f in slot 4 f (the quad's l0), so that DETECT reads the same pixels
        ctx.batch_upload_image(4 * f, lefts[f % args.frames])
    ctx.batch_set_quads([(4 * f, 4 * f, 4 * f, 4 * f) for f in range(B)])
    for f in range(B):   # no carried features: every frame detects (appendNewFeatures on an empty set)
        ctx.batch_set_features(f, np.zeros((0, 2), np.float32), np.zeros(0, np.int32))
    ctx.batch_run(_lib.STAGE_PYRAMID)
    ctx.batch_sync()
    # the detector reads images first .. first + n - 1: a run over the whole table touches the 3 B empty slots too, so the timed
    # run is over a second table that holds the B images contiguously
    ctx2 = _lib.Context(0, W, H, 4096, B)
    ctx2.batch_configure(B, W, H, 1)
    for f in range(B):
        ctx2.batch_upload_image(f, lefts[f % args.frames])
    ctx2.batch_sync()

    def leg_corners():
        for _ in range(args.runs):
            ctx2.corners_batch_run(0, B)
        ctx2.batch_sync()

    def leg_fast():
        for _ in range(args.runs):
            ctx.batch_run(_lib.STAGE_DETECT)
        ctx.batch_sync()

    legs = dict(corners=(leg_corners, []), fast_detect_stage=(leg_fast, []))
    for rep in range(args.repeats + 1):   # (repeat 0 is the warm-up and is not kept)
        for name, (fn, t) in legs.items():
            t0 = time.perf_counter()
            fn()
            if rep:
                t.append(1e3 * (time.perf_counter() - t0) / args.runs)
    for name, (_, t) in legs.items():
        out[name] = stats(t)
        out[name]["per_image_ms"] = out[name]["median_ms"] / B
        print("%-18s %8.3f ms per batch of %d (min %.3f, max %.3f over %d repeats of %d runs) = %.4f ms per image" %
              (name, out[name]["median_ms"], B, out[name]["min_ms"], out[name]["max_ms"], len(t), args.runs, out[name]["per_image_ms"]), flush=True)
    counts = [ctx2.corners_batch_get(f, cap=0)[1] for f in range(min(B, args.frames))]
    out["corners_per_image"] = counts
    print("corners per image:", counts)
    ctx.close()
    ctx2.close()

    if args.calls > 0:
        c = _lib.Context(0, W, H, 4096, 1)
        lat = {}
        for name, fn in (("vocorn_detect", lambda: c.good_features_to_track(lefts[0], 5000, 0.01, 5.0, cap=5000)),
                         ("vo_fast_detect", lambda: c.fast_detect(lefts[0]))):
            for _ in range(10):
                fn()
            t = []
            for _ in range(args.calls):
                t0 = time.perf_counter()
                fn()
                t.append(1e3 * (time.perf_counter() - t0))
            lat[name] = stats(t)
            print("%-18s median %.3f ms  min %.3f  max %.3f over %d calls" % (name, lat[name]["median_ms"], lat[name]["min_ms"], lat[name]["max_ms"], len(t)), flush=True)
        out["latency"] = lat
        c.close()

    if not args.no_cpu:
        import corners_emu as ce
        ce.ref_detect(lefts[0], 5000, 0.01, 5.0)
        t = []
        for k in range(min(args.frames, 4)):
            t0 = time.perf_counter()
            ce.ref_detect(lefts[k], 5000, 0.01, 5.0)
            t.append(1e3 * (time.perf_counter() - t0))
        out["cpu_ref_per_image"] = stats(t)
        print("corners_ref.c      median %.1f ms per image, single-threaded (min %.1f, max %.1f)" % (out["cpu_ref_per_image"]["median_ms"], min(t), max(t)), flush=True)
    if args.rounds:
        import corners_emu as ce
        got = ce.emu_detect([lefts[0]], 5000, 0.01, 5.0, cap=5000, lcap=65536)[0]
        out["rounds_frame0"] = dict(rounds=got[3], candidates=got[2], corners=got[1])
        print("suppression rounds on frame 0 (emulator): %d over %d candidates -> %d corners" % (got[3], got[2], got[1]), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
