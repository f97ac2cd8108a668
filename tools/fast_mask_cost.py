"""What cv::FAST's mask in the frame loop (include/vo_fast_mask.h) costs in the DETECT stage on the MI355X, by the library's own stage
timers (vo_batch_run_timed): one KITTI-shaped rendered frame (1241 x 376) carrying every corner of its unmasked FAST list but the
first `--carried` (default 1 600) -- the load of vo_detect_bucket, which runs the same stage on the same frame -- with the record off
and on, `--repeats` timed runs each after a warm-up; median and range.

    python tools/fast_mask_cost.py [--carried 1600] [--radius 5] [--repeats 30] [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--carried", type=int, default=1600)
    ap.add_argument("--radius", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    from visual_odom_amd import _lib, synth
    world = synth.StereoWorld(seed=20260925)
    lefts, rights, _, _ = world.render_sequence(2)
    h, w = lefts[0].shape
    ctx = _lib.Context(0, w, h, 4096, 1)
    out = dict(w=w, h=h, radius=args.radius, repeats=args.repeats)
    try:
        ctx.set_schedule(pose_waves=2, pose_streams=1, prepare=0, epnp_wide_frames=4)
        corners = ctx.fast_detect(lefts[0])
        carried = np.ascontiguousarray(corners[::max(1, len(corners) // args.carried)][:args.carried])
        out.update(n_fast=len(corners), n_carried=len(carried))
        ctx.batch_configure(4, w, h, 1)
        for i, img in enumerate((lefts[0], rights[0], lefts[1], rights[1])):
            ctx.batch_upload_image(i, img)
        ctx.batch_set_quads([[0, 1, 2, 3]])
        ctx.batch_run(_lib.STAGE_PYRAMID)
        ctx.batch_sync()
        for name, kw in (("off", dict(mode="off")), ("on", dict(radius=args.radius)), ("off_again", dict(mode="off"))):
            ctx.set_fast_topup(**kw)
            t = []
            for k in range(args.repeats + 5):
                ctx.batch_set_features(0, carried, np.zeros(len(carried), np.int32))
                ms = ctx.batch_run_timed(_lib.STAGE_DETECT)
                if k >= 5:
                    t.append(float(ms[1]))
            n = len(ctx.batch_get_features(0)[0])
            out[name] = dict(median_us=1e3 * float(np.median(t)), min_us=1e3 * min(t), max_us=1e3 * max(t), n_bucketed=n)
            print("%-9s DETECT stage %7.1f us (min %.1f, max %.1f over %d runs), %d bucketed" %
                  (name, out[name]["median_us"], out[name]["min_us"], out[name]["max_us"], len(t), n), flush=True)
    finally:
        ctx.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
