"""What rectification at ingest (vo_params.rectify) costs the lock-step loop: 256 sequences, 1241 x 376, resident pairs, at
features_per_bucket 1 (the reference's default: ~300 bucketed points per frame on this rendering) and 6 (~1 600; bench.py's
"~2000" workload setting).

    off  a context WITHOUT maps on pairs remapped beforehand (outside the timer) -- the loop as it always was
    on   a context WITH maps on the raw pairs: the ingest writes raw planes, rectify_kernel follows on the same stream

`--legs off` uses only calls that exist without the feature and runs on an older library (VO_BENCH_ROOT=<checkout>): the
baseline.  Every leg runs `--repeats` times, the legs alternating within a repeat; ms per step = wall time of the timed steps up
to the final synchronise / steps.  The spread of leg `off` over its repeats is the noise figure.  Schedules are pinned (the
same one in every leg and library) so that nothing but the ingest differs.

    python tools/rectify_bench.py [--seqs 256] [--repeats 5] [--legs off,on] [--fpb 1,6] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("VO_BENCH_ROOT", ROOT))   # (another checkout's package: the baseline run)
sys.path.insert(1, os.path.join(ROOT, "tests"))

W, H = 1241, 376


def tri(k, q):
    m = k % (2 * q)
    return m if m <= q else 2 * q - m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--legs", default="off,on")
    ap.add_argument("--fpb", default="1,6", help="features per bucket: 1 = the reference's default (~300 points per frame here), 6 = ~1 600")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=12)
    ap.add_argument("--frames", type=int, default=4, help="distinct rendered pairs (walked forwards and backwards)")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    legs = [l for l in args.legs.split(",") if l]
    import torch
    from rectify_cases import mild_maps, remap_ref
    from visual_odom_amd import _lib, synth
    dev = torch.device("cuda", 0)
    S, Q = args.seqs, args.frames
    world = synth.StereoWorld(seed=20260925)
    L, R, _, _ = world.render_sequence(Q + 1)
    P_l, P_r = world.proj_matrices()
    maps = mild_maps(P_l, W, H)
    raw = [(torch.from_numpy(np.ascontiguousarray(L[k])).to(dev), torch.from_numpy(np.ascontiguousarray(R[k])).to(dev)) for k in range(Q + 1)]
    rect = [(torch.from_numpy(remap_ref(L[k], *maps[0])).to(dev), torch.from_numpy(remap_ref(R[k], *maps[1])).to(dev)) for k in range(Q + 1)]
    torch.cuda.synchronize()
    out = dict(sequences=S, width=W, height=H, repeats=args.repeats, warmup=args.warmup, steps=args.steps, library=_lib.SO_PATH, loads={})
    for fpb in [int(v) for v in args.fpb.split(",")]:
        ctxs, tables = {}, {}
        for leg in legs:
            ctx = _lib.Context(0, W, H, 4096, S)
            if leg == "on":
                ctx.set_params(rectify=maps)
            ctx.set_schedule(pose_waves=2, pose_streams=1, prepare=0, epnp_wide_frames=4)
            ctx.batch_set_detect_params(features_per_bucket=fpb)
            ctx.seq_configure(S, W, H, 3, 4 * (args.warmup + args.steps + 2))
            ctx.batch_set_projection(P_l, P_r)
            src = raw if leg == "on" else rect
            tables[leg] = [ctx.seq_pair_table(range(S), [src[tri(k + s, Q)][0].data_ptr() for s in range(S)],
                                              [src[tri(k + s, Q)][1].data_ptr() for s in range(S)]) for k in range(2 * Q)]
            ctxs[leg] = ctx

        def run(leg):
            ctx = ctxs[leg]
            ctx.seq_sync()
            ctx.seq_reset(-1)

            def step(k):
                ctx.seq_push_pairs(tables[leg][k % (2 * Q)], W, 2)
                ctx.seq_step()
            for k in range(args.warmup + 1):
                step(k)
            ctx.seq_sync()
            t0 = time.perf_counter()
            for k in range(args.warmup + 1, args.warmup + 1 + args.steps):
                step(k)
            ctx.seq_sync()
            dt = time.perf_counter() - t0
            info = ctx.seq_get_trajectory(0)[1]
            return dict(ms_per_step=1e3 * dt / args.steps, frames_per_s=S * args.steps / dt, mean_bucketed=float(info[-args.steps:, 0].mean()),
                        mean_tracked=float(info[-args.steps:, 2].mean()))
        runs = {leg: [] for leg in legs}
        for rep in range(args.repeats):
            for leg in legs:
                r = run(leg)
                runs[leg].append(r)
                print("fpb %d rep %d leg %-3s: %7.3f ms/step  %9.0f frames/s  (%.0f bucketed, %.0f tracked)" %
                      (fpb, rep, leg, r["ms_per_step"], r["frames_per_s"], r["mean_bucketed"], r["mean_tracked"]), flush=True)
        summary = {}
        for leg in legs:
            m = np.array([r["ms_per_step"] for r in runs[leg]])
            summary[leg] = dict(median_ms=float(np.median(m)), min_ms=float(m.min()), max_ms=float(m.max()),
                                spread_pct=float(100 * (m.max() - m.min()) / np.median(m)), mean_bucketed=runs[leg][0]["mean_bucketed"])
            print("fpb %d leg %-3s median %7.3f ms/step  min %7.3f  max %7.3f  spread %.2f %%" %
                  (fpb, leg, summary[leg]["median_ms"], m.min(), m.max(), summary[leg]["spread_pct"]), flush=True)
        out["loads"][str(fpb)] = dict(summary=summary, runs=runs)
        for ctx in ctxs.values():
            ctx.close()
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
