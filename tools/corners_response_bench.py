"""What goodFeaturesToTrack's blockSize / useHarrisDetector (include/vo_corners_response.h) cost on the MI355X, in throughput mode,
and whether the detector without them is what it was.

The workload is tools/corners_bench.py's: `--images` resident 1241 x 376 images (rendered KITTI-shaped frames, `--frames` distinct
ones repeated) at the reference's parameters (5000, 0.01, 5.0); ms per run = wall time of `--runs` back-to-back runs up to the
synchronise / runs, `--repeats` times after a warm-up, the legs alternating within a repeat; the spread over the repeats is the
noise figure.

  plain       vocorn_batch_run: corn_map_kernel
  uploaded    vocmask_batch_run under masks uploaded before the timed window (the left half of every image allowed):
              corn_map_masked_kernel
  resp50      voresp_batch_run at (5, min-eigen), no masks: corn_map_resp_kernel<5, 0>
  resp31      ... at (3, Harris, 0.04): corn_map_resp_kernel<3, 1>
  resp51      ... at (5, Harris, 0.04): corn_map_resp_kernel<5, 1>

THE COMPARISON WITH THE PARENT COMMIT.  `--tree DIR` measures the visual_odom_amd package (with its built libvo_hip.so) of another
checkout; a tree without the response calls runs the first two legs only.  Build both, alternate them in one session --
parent, this, parent, this, `--legs plain,uploaded` -- and take the spread of the parent's own repeats as the margin.

Per-kernel times come from the profiler, in runs of their own, one leg each so that the shared candidate and select kernels are
that leg's:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/corners_response_bench.py --legs resp50 --runs 3 --repeats 1

    python tools/corners_response_bench.py [--tree DIR] [--legs plain,uploaded,resp50,resp31,resp51] [--images 256] [--frames 8] [--runs 10]
                                           [--repeats 5] [--json out.json] [--md profiles/corners_response.md]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

W, H = 1241, 376
RESP = dict(resp50=(5, False), resp31=(3, True), resp51=(5, True))


def stats(t):
    t = np.asarray(t, np.float64)
    return dict(median_ms=float(np.median(t)), min_ms=float(t.min()), max_ms=float(t.max()), n=int(len(t)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--legs", default="plain,uploaded,resp50,resp31,resp51")
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    from visual_odom_amd import _lib, synth
    assert os.path.abspath(_lib.__file__).startswith(os.path.abspath(args.tree)), "the package of --tree is the one measured"
    names = [n for n in args.legs.split(",") if n in ("plain", "uploaded") or (n in RESP and hasattr(_lib, "RESP_EXPORTS"))]
    world = synth.StereoWorld(seed=20260925)
    lefts, _, _, _ = world.render_sequence(args.frames)
    B = args.images
    out = dict(tree=os.path.abspath(args.tree), images=B, w=W, h=H, params=dict(max_corners=5000, quality_level=0.01, min_distance=5.0, k=0.04))

    # one context per table, so that a leg's masks stay what the leg set (max_images = 6 x max_frames: B / 6 frames hold B images)
    def table():
        c = _lib.Context(0, W, H, 4096, (B + 5) // 6)
        c.batch_configure(B, W, H, 1)
        for f in range(B):
            c.batch_upload_image(f, lefts[f % args.frames])
        c.batch_sync()
        return c

    plain = table()
    uploaded = None
    if "uploaded" in names:
        uploaded = table()
        half = np.zeros((H, W), np.uint8)
        half[:, :W // 2] = 255
        for f in range(B):
            uploaded.corners_batch_set_mask(f, half)

    def leg(name):
        ctx = uploaded if name == "uploaded" else plain
        kw = dict(masked=True) if name == "uploaded" else {} if name == "plain" else dict(block_size=RESP[name][0], use_harris=RESP[name][1])

        def fn():
            for _ in range(args.runs):
                ctx.corners_batch_run(0, B, **kw)
            ctx.batch_sync()
        return ctx, fn

    legs = {name: leg(name) + ([],) for name in names}
    n = min(B, args.frames)
    out["corners_per_image"] = {}
    for rep in range(args.repeats + 1):   # (repeat 0 is the warm-up and is not kept)
        for name, (ctx, fn, t) in legs.items():
            t0 = time.perf_counter()
            fn()
            if rep:
                t.append(1e3 * (time.perf_counter() - t0) / args.runs)
            else:
                out["corners_per_image"][name] = [ctx.corners_batch_get(f, cap=0)[1] for f in range(n)]
    for name, (_, _, t) in legs.items():
        out[name] = stats(t)
        out[name]["series_ms"] = [round(v, 4) for v in t]
        print("%-10s %8.3f ms per batch of %d (min %.3f, max %.3f over %d repeats of %d runs)" %
              (name, out[name]["median_ms"], B, out[name]["min_ms"], out[name]["max_ms"], len(t), args.runs), flush=True)
    print("corners per image:", out["corners_per_image"])
    for c in (plain, uploaded):
        if c is not None:
            c.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    if args.md:
        with open(args.md, "w") as f:
            f.write("# Shi-Tomasi detector with a response: measured on the MI355X (tools/corners_response_bench.py)\n\n")
            f.write("%d resident %d x %d images, 5000 / 0.01 / 5.0, %d repeats of %d runs; ms per run of the whole batch.\n\n" % (B, W, H, args.repeats, args.runs))
            f.write("| leg | median | min | max |\n|---|---|---|---|\n")
            for name in legs:
                f.write("| %s | %.3f | %.3f | %.3f |\n" % (name, out[name]["median_ms"], out[name]["min_ms"], out[name]["max_ms"]))
            f.write("\ncorners per image (first frames): %s\n" % json.dumps(out["corners_per_image"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
