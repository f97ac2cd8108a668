"""What the two-image tracker (include/vo_flow.h) costs on the MI355X.

  throughput  voflow_batch_run over `--pairs` (prev, next) pairs of 1241 x 376 with ~2 000 points per frame (bench.py's point
              load), pyramids resident: ms per run = wall time of `--runs` back-to-back runs up to the synchronise / runs.
              Beside it, in the same process on the same table: vo_batch_run(VO_STAGE_LK) with lk_full_chain = 1 over the quads
              (prev, next, prev, next) -- four hops of the product kernel per feature, none retired early -- so that a quarter
              of it is "one hop without the err epilogue" on the same pixels.  The legs alternate within a repeat; the spread of
              a leg over its repeats is the noise figure.
  latency     one synchronous voflow_track (two uploads, two pyramids, one hop, one gather) next to vo_circular_match on four
              images (four uploads, four pyramids, four hops, filter, gather): median and min of `--calls` calls each.

  --win W ...  adds one throughput leg per window: vowin_batch_run(W) (include/vo_flow_win.h) on the same table, alternating with
              the others.  W = 21 there is voflow_batch_run's kernel through the other entry point: the two legs are to agree
              within the spread of `flow`.  With --win the latency part also times vowin_track for each window.

    python tools/flow_bench.py [--pairs 256] [--runs 20] [--repeats 5] [--calls 200] [--win 7 15 21] [--json out.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--frames", type=int, default=4, help="distinct rendered frames the pairs walk over")
    ap.add_argument("--win", type=int, nargs="*", default=[], help="windows to time through vowin_batch_run / vowin_track")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    from visual_odom_amd import _lib, synth
    B, Q = args.pairs, args.frames
    world = synth.StereoWorld(seed=20260925)
    L, R, _, _ = world.render_sequence(Q + 1)
    pts = [np.ascontiguousarray(synth.select_keypoints(L[k], bucket=37, per_bucket=6), np.float32) for k in range(Q)]
    n_max = max(len(p) for p in pts)
    out = dict(pairs=B, width=W, height=H, runs=args.runs, repeats=args.repeats, points_per_frame=float(np.mean([len(p) for p in pts])))

    # ---- throughput ----
    ctx = _lib.Context(0, W, H, max(4096, n_max), B)
    ctx.set_params(lk_full_chain=1)
    ctx.batch_configure(2 * B, W, H, B)
    for f in range(B):   # pair f: consecutive left frames k -> k + 1
        k = f % Q
        ctx.batch_upload_image(2 * f, L[k])
        ctx.batch_upload_image(2 * f + 1, L[k + 1])
        ctx.batch_set_points(f, pts[k])
    ctx.batch_run(_lib.STAGE_PYRAMID)
    ctx.batch_sync()
    ctx.flow_batch_set_pairs([(2 * f, 2 * f + 1) for f in range(B)])
    ctx.batch_set_quads([(2 * f, 2 * f + 1, 2 * f, 2 * f + 1) for f in range(B)])

    def leg_flow():
        ctx.flow_batch_run()

    def leg_chain():
        ctx.batch_run(_lib.STAGE_LK)

    legs = dict(flow=leg_flow, chain4=leg_chain)
    for win in args.win:
        legs["win%d" % win] = lambda win=win: ctx.flow_batch_run(win=win)
    runs = {k: [] for k in legs}
    for rep in range(args.repeats + 1):   # (repeat 0 is the warm-up and is not kept)
        for name, fn in legs.items():
            ctx.batch_sync()
            t0 = time.perf_counter()
            for _ in range(args.runs):
                fn()
            ctx.batch_sync()
            ms = 1e3 * (time.perf_counter() - t0) / args.runs
            if rep:
                runs[name].append(ms)
                print("rep %d leg %-6s %8.3f ms per run" % (rep, name, ms), flush=True)
    nxt, st, err = ctx.flow_batch_get(0, len(pts[0]))
    out["tracked_frame0"] = int((st == 1).sum())
    summ = {}
    for name, v in runs.items():
        v = np.array(v)
        summ[name] = dict(median_ms=float(np.median(v)), min_ms=float(v.min()), max_ms=float(v.max()))
        print("leg %-6s median %8.3f ms per run  min %8.3f  max %8.3f" % (name, np.median(v), v.min(), v.max()), flush=True)
    summ["flow_over_quarter_chain"] = summ["flow"]["median_ms"] / (summ["chain4"]["median_ms"] / 4)
    print("voflow_batch_run / (four-hop chain / 4) = %.3f" % summ["flow_over_quarter_chain"], flush=True)
    out["throughput"] = dict(summary=summ, runs=runs)
    ctx.close()

    # ---- latency ----
    ctx = _lib.Context(0, W, H, max(4096, n_max), 1)
    lat = {}

    def call_flow():
        ctx.flow_track(L[0], L[1], pts[0])

    def call_flow_noerr():
        ctx.flow_track(L[0], L[1], pts[0], want_err=False)

    def call_circ():
        ctx.circular_match(L[0], R[0], L[1], R[1], pts[0])

    calls = [("voflow_track", call_flow), ("voflow_track_no_err", call_flow_noerr), ("vo_circular_match", call_circ)]
    calls += [("vowin_track_%d" % win, lambda win=win: ctx.flow_track(L[0], L[1], pts[0], win=win)) for win in args.win]
    for name, fn in calls:
        for _ in range(20):
            fn()
        t = []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            fn()
            t.append(1e3 * (time.perf_counter() - t0))
        t = np.array(t)
        lat[name] = dict(median_ms=float(np.median(t)), min_ms=float(t.min()), p90_ms=float(np.percentile(t, 90)))
        print("%-20s median %7.3f ms  min %7.3f  p90 %7.3f  (%d points)" % (name, np.median(t), t.min(), np.percentile(t, 90), len(pts[0])), flush=True)
    out["latency"] = lat
    ctx.close()
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
