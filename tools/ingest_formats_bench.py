"""Throughput of the lock-step loop fed with interleaved (VO_FMT_GRAY8_X2) and colour (VO_FMT_BGR8) frames as they are, against
the gray loop with the conversion done by the caller: 256 sequences, 640 x 480 (the reference sensor's size,
rgbd_standalone.cpp), reference-default detection load, page-locked sources.

    a  GRAY8, planes already split (host conversion outside the timer) -- the link-byte equal of b
    b  GRAY8_X2, the interleaved buffers handed over as they are (left = buf, right = buf + 1)
    c  GRAY8 with the host de-interleave (numpy slicing copy into page-locked planes) INSIDE the loop
    d  BGR8 as it is
    e  GRAY8 with the host colour conversion (numpy int32, the formula of visual_odom_amd.run.bgr_to_gray) inside the loop

Legs a, c and e use only calls that exist without the feature (`--legs a,c,e` runs on an older library: the baseline).  Every
leg runs `--repeats` times, the legs alternating within a repeat; frames/s = sequences x timed steps / wall time of the timed
steps up to the final synchronise.  The spread of leg a over its repeats is the noise figure.  The library's schedule is left
to settle (on leg a's data, before anything is timed; the settled schedule is process-wide for the shape) so that all legs
run the same one.

    python tools/ingest_formats_bench.py [--seqs 256] [--repeats 5] [--legs a,b,c,d,e] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("VO_BENCH_ROOT", ROOT))   # (another checkout's package: the baseline run)

W, H = 640, 480
FMT_GRAY8, FMT_GRAY8_X2, FMT_BGR8 = 0, 1, 2
SLOTS = 6   # page-locked destination slots of the host-converting legs: the host runs at most 4 steps ahead of the device


def tri(k, q):
    m = k % (2 * q)
    return m if m <= q else 2 * q - m


def gray_of_bgr(bgr):
    b, g, r = bgr[..., 0].astype(np.int32), bgr[..., 1].astype(np.int32), bgr[..., 2].astype(np.int32)
    return ((b * 1868 + g * 9617 + r * 4899 + (1 << 13)) >> 14).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--legs", default="a,b,c,d,e")
    ap.add_argument("--steps", type=int, default=150, help="timed steps of the legs a, b, d")
    ap.add_argument("--steps-c", type=int, default=40)
    ap.add_argument("--steps-e", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=12)
    ap.add_argument("--frames", type=int, default=4, help="distinct rendered pairs (walked forwards and backwards)")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    legs = [l for l in args.legs.split(",") if l]
    import torch
    from visual_odom_amd import _lib, synth
    S, Q = args.seqs, args.frames
    world = synth.StereoWorld(seed=640480, width=W, height=H, fx=420.0, cx=319.5, cy=239.5, bf=-220.0, tex_size=1024)
    L, R, _, _ = world.render_sequence(Q + 1)
    P_l, P_r = world.proj_matrices()
    rng = np.random.default_rng(1)

    def colour(g):   # channels that differ; what the camera would have delivered
        g = g.astype(np.float64)
        return np.stack([np.clip(g * 0.9 + 30 + rng.integers(-5, 6, g.shape), 0, 255), np.clip(g * 1.04 - 6, 0, 255),
                         np.clip(g * 0.8 + 20 + rng.integers(-7, 8, g.shape), 0, 255)], axis=-1).astype(np.uint8)

    def pinned(a):
        return torch.from_numpy(np.ascontiguousarray(a)).pin_memory()
    # sources, page-locked, shared by the sequences like bench.py's (sequence s shows pair tri(k + s))
    y8i = [pinned(np.stack([L[k], R[k]], axis=-1)) for k in range(Q + 1)]                      # (h, w, 2): one buffer per pair
    bgr = [(pinned(colour(L[k])), pinned(colour(R[k]))) for k in range(Q + 1)] if set(legs) & {"d", "e"} else None
    planes = [(pinned(L[k]), pinned(R[k])) for k in range(Q + 1)]                                 # leg a: split outside the timer
    dst = torch.empty((SLOTS, S, 2, H, W), dtype=torch.uint8).pin_memory() if set(legs) & {"c", "e"} else None
    dst_np = dst.numpy() if dst is not None else None

    ctxs = {}

    def context(fmt):
        if fmt not in ctxs:
            ctx = _lib.Context(0, W, H, 4096, S)
            if fmt != FMT_GRAY8:
                ctx.set_params(input_format=fmt)
            ctx.set_schedule()
            ctx.batch_set_detect_params()   # the reference's defaults
            ctx.seq_configure(S, W, H, 3, 1400)
            ctx.batch_set_projection(P_l, P_r)
            ctxs[fmt] = ctx
        return ctxs[fmt]

    def table(ctx, ptrs_of, k):
        p = [ptrs_of(tri(k + s, Q)) for s in range(S)]
        return ctx.seq_pair_table(range(S), [a for a, _ in p], [b for _, b in p])

    def make_leg(leg):
        """-> (ctx, step(k), link bytes per step)"""
        if leg in ("a", "b", "d"):
            fmt, ptrs_of, stride = {"a": (FMT_GRAY8, lambda i: (planes[i][0].data_ptr(), planes[i][1].data_ptr()), W),
                                    "b": (FMT_GRAY8_X2, lambda i: (y8i[i].data_ptr(), y8i[i].data_ptr() + 1), 2 * W),
                                    "d": (FMT_BGR8, lambda i: (bgr[i][0].data_ptr(), bgr[i][1].data_ptr()), 3 * W)}[leg]
            ctx = context(fmt)
            tables = [table(ctx, ptrs_of, k) for k in range(2 * Q)]

            def step(k):
                ctx.seq_push_pairs(tables[k % (2 * Q)], stride, 1)
                ctx.seq_step()
            return ctx, step, S * 2 * W * H * (3 if leg == "d" else 1)
        ctx = context(FMT_GRAY8)
        base = dst.data_ptr()
        tables = [ctx.seq_pair_table(range(S), [base + ((sl * S + s) * 2) * W * H for s in range(S)],
                                     [base + ((sl * S + s) * 2 + 1) * W * H for s in range(S)]) for sl in range(SLOTS)]
        y8i_np = [t.numpy() for t in y8i]
        bgr_np = [(a.numpy(), b.numpy()) for a, b in bgr] if bgr else None

        def step(k):
            sl = k % SLOTS
            for s in range(S):   # every sequence's own frame is converted, as a caller with S cameras has to
                i = tri(k + s, Q)
                if leg == "c":
                    dst_np[sl, s, 0] = y8i_np[i][..., 0]
                    dst_np[sl, s, 1] = y8i_np[i][..., 1]
                else:
                    dst_np[sl, s, 0] = gray_of_bgr(bgr_np[i][0])
                    dst_np[sl, s, 1] = gray_of_bgr(bgr_np[i][1])
            ctx.seq_push_pairs(tables[sl], W, 1)
            ctx.seq_step()
        return ctx, step, S * 2 * W * H

    def run(leg, K):
        ctx, step, link_bytes = make_leg(leg)
        ctx.seq_sync()
        ctx.seq_reset(-1)
        for k in range(args.warmup + 1):
            step(k)
        ctx.seq_sync()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(args.warmup + 1, args.warmup + 1 + K):
            step(k)
        ctx.seq_sync()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        info = ctx.seq_get_trajectory(0)[1]
        return dict(frames_per_s=S * K / dt, ms_per_step=1e3 * dt / K, link_GB_per_s=link_bytes * K / dt / 1e9,
                    mean_bucketed=float(info[-K:, 0].mean()), mean_tracked=float(info[-K:, 2].mean()))

    # settle the schedule of every context that will be timed, before anything is timed
    settle = {}
    for leg in legs:
        ctx, step, _ = make_leg(leg)
        if id(ctx) in settle:
            continue
        if leg in ("c", "e") and "a" in legs:
            continue   # (the gray context settles on leg a's cheap steps)
        k = 0
        step(k)
        while (ctx.get_schedule()["settling"] or k < 4) and k < 560:
            k += 1
            step(k)
        ctx.seq_sync()
        settle[id(ctx)] = dict(leg=leg, steps=k + 1, schedule=ctx.get_schedule())
    K_of = dict(a=args.steps, b=args.steps, d=args.steps, c=args.steps_c, e=args.steps_e)
    runs = {leg: [] for leg in legs}
    for rep in range(args.repeats):
        for leg in legs:
            r = run(leg, K_of[leg])
            runs[leg].append(r)
            print("rep %d leg %s: %9.0f frames/s  %7.3f ms/step  %6.2f GB/s over the link" % (rep, leg, r["frames_per_s"], r["ms_per_step"],
                                                                                            r["link_GB_per_s"]), flush=True)
    print("\nleg  frames/s: median      min      max   spread%   GB/s(median)  points bucketed / tracked per frame")
    summary = {}
    for leg in legs:
        f = np.array([r["frames_per_s"] for r in runs[leg]])
        g = float(np.median([r["link_GB_per_s"] for r in runs[leg]]))
        summary[leg] = dict(median=float(np.median(f)), min=float(f.min()), max=float(f.max()), spread_pct=float(100 * (f.max() - f.min()) / np.median(f)),
                            link_GB_per_s=g, timed_steps=K_of[leg])
        print("%-3s %18.0f %8.0f %8.0f %8.2f %12.2f   %.0f / %.0f" % (leg, summary[leg]["median"], f.min(), f.max(), summary[leg]["spread_pct"], g,
                                                                      runs[leg][0]["mean_bucketed"], runs[leg][0]["mean_tracked"]))
    out = dict(sequences=S, width=W, height=H, repeats=args.repeats, warmup=args.warmup, library=_lib.SO_PATH, settle=list(settle.values()),
               summary=summary, runs=runs)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)
    for ctx in ctxs.values():
        ctx.close()


if __name__ == "__main__":
    main()
