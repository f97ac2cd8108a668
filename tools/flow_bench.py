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

  --guess      what OPTFLOW_USE_INITIAL_FLOW buys (include/vo_flow_flags.h), at 21 x 21 through the batch calls on the same pairs:
                (a)   vowin_batch_run(21) at lk_max_level 3;
                (b)   voflag_batch_run(21, USE_INITIAL_FLOW) at lk_max_level 0 with (a)'s answer as the guess -- a PERFECT
                      prediction, i.e. an upper bound on the gain;
                (c)   the same at lk_max_level 3;
                (a0)  vowin_batch_run(21) at lk_max_level 0, what dropping the levels without a guess gives;
                (eig) voflag_batch_run(21, GET_MIN_EIGENVALS) at lk_max_level 3 against (a): no epilogue, one sqrt and divide.
              A run leaves its results where the next run's guesses are read, so every timed run here is ONE run between two
              synchronisations with the guesses written again before it (untimed); `--runs` x `--repeats` of them per leg.  Each
              leg also reports how many of the points it tracks end within 0.05 px of (a)'s position.  lk_max_level is part of
              the pyramid plan, so the level-0 legs run on a table of their own after the level-3 legs, not alternating with them.
  --skip-base  with --guess: only that section.

    python tools/flow_bench.py [--pairs 256] [--runs 20] [--repeats 5] [--calls 200] [--win 7 15 21] [--guess] [--json out.json]
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


def guess_legs(args, _lib, L, pts, n_max):
    """the --guess section (see the module's text)"""
    B, Q = args.pairs, args.frames
    ctx = _lib.Context(0, W, H, max(4096, n_max), B)
    counts = [len(pts[f % Q]) for f in range(B)]

    def table(level):
        ctx.set_params(lk_max_level=level)
        ctx.batch_configure(2 * B, W, H, B)
        for f in range(B):
            k = f % Q
            ctx.batch_upload_image(2 * f, L[k])
            ctx.batch_upload_image(2 * f + 1, L[k + 1])
            ctx.batch_set_points(f, pts[k])
        ctx.batch_run(_lib.STAGE_PYRAMID)
        ctx.batch_sync()
        ctx.flow_batch_set_pairs([(2 * f, 2 * f + 1) for f in range(B)])

    def results():
        ctx.batch_sync()
        return [ctx.flow_batch_get(f, n) for f, n in enumerate(counts)]

    def timed(name, run, guesses=None):
        t = []
        for i in range(1 + args.runs * args.repeats):   # (run 0 is the warm-up and is not kept)
            if guesses is not None:
                for f, g in enumerate(guesses):
                    ctx.flow_batch_set_guess(f, g)
            ctx.batch_sync()
            t0 = time.perf_counter()
            run()
            ctx.batch_sync()
            if i:
                t.append(1e3 * (time.perf_counter() - t0))
        t = np.array(t)
        return dict(median_ms=float(np.median(t)), min_ms=float(t.min()), max_ms=float(t.max()), n_runs=len(t)), results()

    def agreement(res, ref):
        tracked = within = 0
        for (nxt, st, _), (rn, _, _) in zip(res, ref):
            ok = st == 1
            tracked += int(ok.sum())
            within += int((np.abs(nxt[ok] - rn[ok]).max(1) <= 0.05).sum()) if ok.any() else 0
        return dict(tracked=tracked, within_0p05_of_a=within)

    legs = {}
    table(3)
    legs["a_win21_level3"], ref = timed("a", lambda: ctx.flow_batch_run(win=21))
    answer = [np.ascontiguousarray(r[0]) for r in ref]
    legs["c_guess_level3"], rc = timed("c", lambda: ctx.flow_batch_run(win=21, guess=True), answer)
    legs["eig_level3"], re = timed("eig", lambda: ctx.flow_batch_run(win=21, min_eigenvals=True))
    table(0)
    legs["a0_win21_level0"], r0 = timed("a0", lambda: ctx.flow_batch_run(win=21))
    legs["b_guess_level0"], rb = timed("b", lambda: ctx.flow_batch_run(win=21, guess=True), answer)
    for name, res in (("a_win21_level3", ref), ("c_guess_level3", rc), ("eig_level3", re), ("a0_win21_level0", r0), ("b_guess_level0", rb)):
        legs[name].update(agreement(res, ref))
        print("guess leg %-16s median %8.3f ms  min %8.3f  max %8.3f  tracked %d  within 0.05 px of (a) %d" %
              (name, legs[name]["median_ms"], legs[name]["min_ms"], legs[name]["max_ms"], legs[name]["tracked"], legs[name]["within_0p05_of_a"]), flush=True)
    legs["points"] = int(sum(counts))
    ctx.close()
    if args.calls > 0:   # the synchronous call: what the guess's own copy and the flags cost per call (lk_max_level 3)
        ctx = _lib.Context(0, W, H, max(4096, n_max), 1)
        g = answer[0]
        calls = [("vowin_track_21", lambda: ctx.flow_track(L[0], L[1], pts[0], win=21)),
                 ("voflag_track_21_guess", lambda: ctx.flow_track(L[0], L[1], pts[0], win=21, guess=g)),
                 ("voflag_track_21_min_eig", lambda: ctx.flow_track(L[0], L[1], pts[0], win=21, min_eigenvals=True))]
        lat = {}
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
            print("%-24s median %7.3f ms  min %7.3f  p90 %7.3f  (%d points)" % (name, np.median(t), t.min(), np.percentile(t, 90), len(pts[0])), flush=True)
        legs["latency"] = lat
        ctx.close()
    return legs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--frames", type=int, default=4, help="distinct rendered frames the pairs walk over")
    ap.add_argument("--win", type=int, nargs="*", default=[], help="windows to time through vowin_batch_run / vowin_track")
    ap.add_argument("--guess", action="store_true", help="the USE_INITIAL_FLOW / GET_MIN_EIGENVALS legs")
    ap.add_argument("--skip-base", action="store_true", help="with --guess: skip the throughput and latency sections")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    from visual_odom_amd import _lib, synth
    B, Q = args.pairs, args.frames
    world = synth.StereoWorld(seed=20260925)
    L, R, _, _ = world.render_sequence(Q + 1)
    pts = [np.ascontiguousarray(synth.select_keypoints(L[k], bucket=37, per_bucket=6), np.float32) for k in range(Q)]
    n_max = max(len(p) for p in pts)
    out = dict(pairs=B, width=W, height=H, runs=args.runs, repeats=args.repeats, points_per_frame=float(np.mean([len(p) for p in pts])))

    if args.guess:
        out["guess"] = guess_legs(args, _lib, L, pts, n_max)
    if args.guess and args.skip_base:
        if args.json:
            with open(args.json, "w") as fh:
                json.dump(out, fh, indent=1)
        return

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
