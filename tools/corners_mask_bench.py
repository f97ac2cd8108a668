"""What the Shi-Tomasi detector's mask argument (include/vo_corners_mask.h) costs on the MI355X, in throughput mode.

The workload is tools/corners_bench.py's: `--images` resident 1241 x 376 images (rendered KITTI-shaped frames, `--frames` distinct
ones repeated) at the reference's parameters (5000, 0.01, 5.0); ms per run = wall time of `--runs` back-to-back runs up to the
synchronise / runs, `--repeats` times after a warm-up, the legs alternating within a repeat; the spread over the repeats is the
noise figure.

  (a) plain       vocorn_batch_run: the unmasked kernels.  The same leg of tools/corners_bench.py at the parent commit is the
                  comparison (the kernels are the same: the two must agree within the run-to-run spread).
  (b) uploaded    vocmask_batch_run under masks uploaded before the timed window: the left half of every image allowed.
  (c) kept        per run: vocmask_batch_set_kept for every image (`--kept` points, radius `--radius`: the points cross the host
                  link, the masks are built on the device) + vocmask_batch_run.
  (c') kept-run   vocmask_batch_run alone under the masks (c) left.

Per-kernel times come from the profiler, in a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/corners_mask_bench.py --runs 3 --repeats 1
(kernel names: corn_map_kernel, corn_map_masked_kernel, corn_cand_kernel, corn_select_kernel, corn_disc_kernel).

    python tools/corners_mask_bench.py [--images 256] [--frames 8] [--runs 10] [--repeats 5] [--json out.json] [--md profiles/corners_mask.md]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

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
    ap.add_argument("--kept", type=int, default=1500)
    ap.add_argument("--radius", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    from visual_odom_amd import _lib, synth
    world = synth.StereoWorld(seed=20260925)
    lefts, _, _, _ = world.render_sequence(args.frames)
    B = args.images
    out = dict(images=B, w=W, h=H, params=dict(max_corners=5000, quality_level=0.01, min_distance=5.0), kept=args.kept, radius=args.radius)

    # one context per leg, so that each leg's masks stay what the leg set (max_images = 6 x max_frames: B / 6 frames hold B images)
    def table():
        c = _lib.Context(0, W, H, 4096, (B + 5) // 6)
        c.batch_configure(B, W, H, 1)
        for f in range(B):
            c.batch_upload_image(f, lefts[f % args.frames])
        c.batch_sync()
        return c

    plain, uploaded, kept = table(), table(), table()
    half = np.zeros((H, W), np.uint8)
    half[:, :W // 2] = 255
    for f in range(B):
        uploaded.corners_batch_set_mask(f, half)
    rng = np.random.default_rng(7)
    pts = [np.stack([rng.uniform(0, W, args.kept), rng.uniform(0, H, args.kept)], axis=1).astype(np.float32) for _ in range(args.frames)]

    def leg_plain():
        for _ in range(args.runs):
            plain.corners_batch_run(0, B)
        plain.batch_sync()

    def leg_uploaded():
        for _ in range(args.runs):
            uploaded.corners_batch_run(0, B, masked=True)
        uploaded.batch_sync()

    def leg_kept():
        for _ in range(args.runs):
            for f in range(B):
                kept.corners_batch_set_kept(f, pts[f % args.frames], args.radius)
            kept.corners_batch_run(0, B, masked=True)
        kept.batch_sync()

    def leg_kept_run():
        for _ in range(args.runs):
            kept.corners_batch_run(0, B, masked=True)
        kept.batch_sync()

    legs = dict(plain=(leg_plain, []), uploaded=(leg_uploaded, []), kept=(leg_kept, []), kept_run=(leg_kept_run, []))
    for rep in range(args.repeats + 1):   # (repeat 0 is the warm-up and is not kept)
        for name, (fn, t) in legs.items():
            t0 = time.perf_counter()
            fn()
            if rep:
                t.append(1e3 * (time.perf_counter() - t0) / args.runs)
    for name, (_, t) in legs.items():
        out[name] = stats(t)
        print("%-10s %8.3f ms per batch of %d (min %.3f, max %.3f over %d repeats of %d runs)" %
              (name, out[name]["median_ms"], B, out[name]["min_ms"], out[name]["max_ms"], len(t), args.runs), flush=True)
    n = min(B, args.frames)
    out["corners_per_image"] = dict(plain=[plain.corners_batch_get(f, cap=0)[1] for f in range(n)],
                                    uploaded=[uploaded.corners_batch_get(f, cap=0)[1] for f in range(n)],
                                    kept=[kept.corners_batch_get(f, cap=0)[1] for f in range(n)])
    print("corners per image:", out["corners_per_image"])
    for c in (plain, uploaded, kept):
        c.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    if args.md:
        with open(args.md, "w") as f:
            f.write("# Shi-Tomasi detector under a mask: measured on the MI355X (tools/corners_mask_bench.py)\n\n")
            f.write("%d resident %d x %d images, 5000 / 0.01 / 5.0, %d repeats of %d runs; ms per run of the whole batch.\n\n" % (B, W, H, args.repeats, args.runs))
            f.write("| leg | median | min | max |\n|---|---|---|---|\n")
            for name in legs:
                f.write("| %s | %.3f | %.3f | %.3f |\n" % (name, out[name]["median_ms"], out[name]["min_ms"], out[name]["max_ms"]))
            f.write("\ncorners per image (first frames): %s\n" % json.dumps(out["corners_per_image"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
