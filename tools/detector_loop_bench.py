"""What the frame loop costs with each detector (include/vo_detector.h) on the MI355X, and whether the FAST loop is what it was.

KITTI-shaped rendered frames (1241 x 376), the reference's load (FAST 20 / nonmax, goodFeaturesToTrack 5000 / 0.01 / 5.0 / 3 /
false / 0.04, re-detect below 2000, bucket = rows / 10, one feature per bucket).  Per leg `--repeats` repeats of `--runs` frames or
steps after a warm-up; the median and the range over the repeats are reported, the range being the noise figure.

  sync        StereoOdometry on the kept pair (vo_detect_bucket + vo_track_frame per frame): ms per frame
  seq<S>      the lock-step loop with S sequences, device-resident pairs, ring 3, the schedule the library settles on (warm-up lasts
              until it has settled; the sequences then start over): ms per step, and the settled schedule

THE COMPARISON WITH THE PARENT COMMIT.  `--tree DIR` measures the visual_odom_amd package (with its built libvo_hip.so) of another
checkout; a tree without vodet_* runs the FAST legs only.  Build both, alternate them in one session -- parent, this, parent, this,
`--detectors fast` -- and hold every median of this commit against the parent's largest repeat (DESIGN 3.14's rule).

`--topup-radius R` adds a third column where the tree has votop_* (include/vo_topup.h): shi_tomasi with the top-up under the disc mask,
radius R, of the carried points -- named shi_tomasi+top in the tables.  The Shi-Tomasi legs beside it run with the top-up off.

`--fast-topup-radius R` adds a column where the tree has vofm_* (include/vo_fast_mask.h): fast with cv::FAST's call under the same disc
mask -- named fast+top.  The FAST legs beside it run with the record off.

    python tools/detector_loop_bench.py [--tree DIR] [--detectors fast,shi_tomasi] [--topup-radius R] [--fast-topup-radius R] [--legs sync,seq256,seq64,seq8]
                                        [--runs 10] [--repeats 5] [--json out.json] [--md profiles/detector_loop.md]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, Q = 1241, 376, 4


def stats(t):
    t = np.asarray(t, np.float64)
    return dict(median_ms=float(np.median(t)), min_ms=float(t.min()), max_ms=float(t.max()), n=int(len(t)), series_ms=[round(float(v), 4) for v in t])


def tri(k, q):   # 0, 1, .., q, q - 1, .., 1, 0, 1, ..: consecutive pairs are always neighbours of the rendered drive
    k %= 2 * q
    return k if k <= q else 2 * q - k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--detectors", default="fast,shi_tomasi")
    ap.add_argument("--topup-radius", type=int, default=None)
    ap.add_argument("--fast-topup-radius", type=int, default=None)
    ap.add_argument("--legs", default="sync,seq256,seq64,seq8")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    from visual_odom_amd import _lib, odometry, synth
    assert os.path.abspath(_lib.__file__).startswith(os.path.abspath(args.tree)), "the package of --tree is the one measured"
    has_det = hasattr(_lib, "DET_EXPORTS")
    detectors = [d for d in args.detectors.split(",") if d == "fast" or (d == "shi_tomasi" and has_det)]
    if args.topup_radius is not None and has_det and hasattr(_lib, "TOPUP_EXPORTS"):
        detectors.append("shi_tomasi+top")
    if args.fast_topup_radius is not None and "fast" in detectors and hasattr(_lib, "FAST_MASK_EXPORTS"):
        detectors.insert(detectors.index("fast") + 1, "fast+top")
    top_kw = lambda det: ({} if not det.endswith("+top") else dict(fast_topup_radius=args.fast_topup_radius) if det.startswith("fast") else
                          dict(topup_radius=args.topup_radius))
    world = synth.StereoWorld(seed=20260925)
    lefts, rights, _, _ = world.render_sequence(Q + 1)
    P_l, P_r = world.proj_matrices()
    dev = torch.device("cuda", 0)
    src = [(torch.from_numpy(np.ascontiguousarray(lefts[k])).to(dev), torch.from_numpy(np.ascontiguousarray(rights[k])).to(dev)) for k in range(Q + 1)]
    torch.cuda.synchronize()
    ptrs = [(a.data_ptr(), b.data_ptr()) for a, b in src]
    out = dict(tree=os.path.abspath(args.tree), w=W, h=H, runs=args.runs, repeats=args.repeats, legs={})

    def sync_leg(det):
        vo = odometry.StereoOdometry(P_l, P_r, max_w=W, max_h=H, **(dict(detector=det.split("+")[0], **top_kw(det)) if has_det else {}))
        try:
            k = 0
            for _ in range(2 * args.runs):   # warm-up: the schedule of the synchronous calls settles in their first frames
                vo.process(lefts[tri(k, Q)], rights[tri(k, Q)])
                k += 1
            t = []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                for _ in range(args.runs):
                    vo.process(lefts[tri(k, Q)], rights[tri(k, Q)])
                    k += 1
                t.append(1e3 * (time.perf_counter() - t0) / args.runs)
            r = stats(t)
            r["n_bucketed"] = [rec["n_bucketed"] for rec in vo.log[-4:]]
            return r
        finally:
            vo.close()

    def seq_leg(det, S):
        ctx = _lib.Context(0, W, H, 4096, S)
        try:
            ctx.batch_set_detect_params(features_per_bucket=1)
            if has_det:
                ctx.set_detector(det.split("+")[0])
            if det == "fast+top":
                ctx.set_fast_topup(radius=args.fast_topup_radius)
            elif det.endswith("+top"):
                ctx.set_topup(radius=args.topup_radius)
            ctx.seq_configure(S, W, H, 3, (args.repeats + 3) * args.runs + 600)
            ctx.batch_set_projection(P_l, P_r)
            tables = [ctx.seq_pair_table(range(S), [ptrs[tri(k + s, Q)][0] for s in range(S)], [ptrs[tri(k + s, Q)][1] for s in range(S)])
                      for k in range(2 * Q)]

            def step(k):
                ctx.seq_push_pairs(tables[k % (2 * Q)], W, 2)
                ctx.seq_step()

            k = 0
            for _ in range(args.runs + 1):
                step(k)
                k += 1
            extra = 0
            while ctx.get_schedule()["settling"] and extra < 520:
                step(k)
                k += 1
                extra += 1
            ctx.seq_sync()
            ctx.seq_reset(-1)
            k = 0
            for _ in range(args.runs + 1):
                step(k)
                k += 1
            ctx.seq_sync()
            t = []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                for _ in range(args.runs):
                    step(k)
                    k += 1
                ctx.seq_sync()
                t.append(1e3 * (time.perf_counter() - t0) / args.runs)
            r = stats(t)
            s = ctx.get_schedule()
            r["schedule"] = "%d,%d,%d,%d" % (s["pose_waves"], s["pose_streams"], s["prepare"], s["epnp_wide_frames"])
            r["settling_steps"] = extra
            info = ctx.seq_get_trajectory(0)[1]
            r["n_bucketed"] = [int(v) for v in info[-4:, 0]]
            r["overflow"] = int(np.any(info[:, 7] != 0))
            return r
        finally:
            ctx.close()

    for leg in args.legs.split(","):
        for det in detectors:
            r = sync_leg(det) if leg == "sync" else seq_leg(det, int(leg[3:]))
            out["legs"]["%s/%s" % (leg, det)] = r
            print("%-8s %-14s %8.3f ms (min %.3f, max %.3f over %d repeats of %d)%s  bucketed %s" %
                  (leg, det, r["median_ms"], r["min_ms"], r["max_ms"], r["n"], args.runs, "  schedule " + r["schedule"] if "schedule" in r else "",
                   r["n_bucketed"]), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    if args.md:
        with open(args.md, "w") as f:
            f.write("# The frame loop with each detector: measured on the MI355X (tools/detector_loop_bench.py)\n\n")
            f.write("%d x %d rendered frames, the reference's load, %d repeats of %d frames / steps; ms per frame (sync) or per step (seq<S>: S "
                    "sequences, device-resident pairs, the settled schedule).\n\n" % (W, H, args.repeats, args.runs))
            f.write("| leg | detector | median | min | max | schedule | bucketed (last frames) |\n|---|---|---|---|---|---|---|\n")
            for name, r in out["legs"].items():
                leg, det = name.split("/")
                f.write("| %s | %s | %.3f | %.3f | %.3f | %s | %s |\n" % (leg, det, r["median_ms"], r["min_ms"], r["max_ms"], r.get("schedule", "-"),
                                                                         r["n_bucketed"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
