"""Argument sweep over the five calls of include/vo_flow.h: NULL pointers, n < 0, n > capacity, sizes beyond the context's, short
strides, pair indices outside the table, frames beyond the table, calls in the wrong state.  Every such call must come back with
the documented code -- never a fault, never a silent success -- and leave vo_last_error filled.  Run as a SCRIPT in a child
process by tests/test_gpu_flow.py (a fault would otherwise take the test session down with it); prints one JSON object
{"checked": n, "covered": [...], "failures": [...]} and exits 0 iff there is no failure.  Needs a GPU (vo_create)."""
import sys

import numpy as np

from flow_sweep_common import ARG, CAP, FRAMES, OK, SENT, STATE, H, W, Sweep, _lib, vp


def main():
    s = Sweep()
    ctx, h, fails, expect = s.ctx, s.h, s.fails, s.expect
    img, pts, out, st, err, idx, n_out, pn = s.img, s.pts, s.out, s.st, s.err, s.idx, s.n_out, s.pn
    I, P, O, S, E, K = s.pointers

    # ---- voflow_track ----
    T = "voflow_track"
    expect(T, ARG, None, I, I, W, H, W, P, 4, O, S, E)
    expect(T, ARG, h, None, I, W, H, W, P, 4, O, S, E)
    expect(T, ARG, h, I, None, W, H, W, P, 4, O, S, E)
    expect(T, ARG, h, I, I, W, H, W, None, 4, O, S, E)
    expect(T, ARG, h, I, I, W, H, W, P, 4, None, S, E)
    expect(T, ARG, h, I, I, W, H, W, P, 4, O, None, E)
    expect(T, ARG, h, I, I, W, H, W, P, -1, O, S, E)
    expect(T, ARG, h, I, I, W, H, W, P, CAP + 1, O, S, E)
    expect(T, ARG, h, I, I, W + 8, H, W + 8, P, 4, O, S, E)
    expect(T, ARG, h, I, I, W, H + 8, W, P, 4, O, S, E)
    expect(T, ARG, h, I, I, 16, H, W, P, 4, O, S, E)
    expect(T, ARG, h, I, I, W, H, W - 1, P, 4, O, S, E)
    expect(T, OK, h, I, I, W, H, W, P, 0, O, S, E)         # n == 0: VO_OK, nothing written
    expect(T, OK, h, I, I, W, H, W, None, 0, None, None, None)
    if (out != SENT).any() or (st != 9).any() or (err != SENT).any():
        fails.append("a refused / empty voflow_track call wrote to its outputs")
    expect(T, OK, h, I, I, W, H, W, P, 4, O, S, None)      # err is optional
    expect(T, OK, h, I, I, W, H, W, P, CAP, O, S, E)       # n == max_pts is allowed
    if (out[CAP:] != SENT).any() or (st[CAP:] != 9).any() or (err[CAP:] != SENT).any():
        fails.append("voflow_track wrote beyond n")
    ctx.set_params(input_format=_lib.FMT_BGR8)
    expect(T, ARG, h, I, I, 100, H, 299, P, 4, O, S, E)    # stride below 3 bytes per pixel
    ctx.set_params(input_format=_lib.FMT_GRAY8)

    # ---- voflow_feature_tracking ----
    F = "voflow_feature_tracking"
    expect(F, ARG, None, I, I, W, H, W, P, 4, O, S, E, K, pn)
    expect(F, ARG, h, None, I, W, H, W, P, 4, O, S, E, K, pn)
    expect(F, ARG, h, I, None, W, H, W, P, 4, O, S, E, K, pn)
    expect(F, ARG, h, I, I, W, H, W, None, 4, O, S, E, K, pn)
    expect(F, ARG, h, I, I, W, H, W, P, 4, None, S, E, K, pn)
    expect(F, ARG, h, I, I, W, H, W, P, 4, O, None, E, K, pn)
    expect(F, ARG, h, I, I, W, H, W, P, 4, O, S, E, K, None)
    expect(F, ARG, h, I, I, W, H, W, P, -1, O, S, E, K, pn)
    expect(F, ARG, h, I, I, W, H, W, P, CAP + 1, O, S, E, K, pn)
    expect(F, ARG, h, I, I, W + 8, H, W + 8, P, 4, O, S, E, K, pn)
    expect(F, ARG, h, I, I, W, H, W - 1, P, 4, O, S, E, K, pn)
    if n_out.value != -5 or (idx != -5).any():
        fails.append("a refused voflow_feature_tracking call wrote to its outputs")
    expect(F, OK, h, I, I, W, H, W, P, 0, O, S, E, K, pn)
    if n_out.value != -5:
        fails.append("voflow_feature_tracking with n == 0 wrote n_out")
    expect(F, OK, h, I, I, W, H, W, vp(pts.copy()), 4, O, S, None, None, pn)  # err and keep_idx are optional

    # ---- throughput mode ----
    SP, RUN, GET = "voflow_batch_set_pairs", "voflow_batch_run", "voflow_batch_get"
    pairs = np.array([[0, 1], [1, 2]], np.int32)
    fresh = _lib.Context(0, W, H, CAP, FRAMES)
    expect(SP, STATE, fresh.h, vp(pairs), 2)               # no table configured
    expect(RUN, STATE, fresh.h)
    expect(GET, STATE, fresh.h, 0, O, S, E, 4)             # nothing has run
    fresh.close()
    ctx.batch_configure(3, W, H, 2)
    expect(RUN, STATE, h)                                  # configured, no pairs
    expect(SP, ARG, None, vp(pairs), 2)
    expect(SP, ARG, h, None, 2)
    expect(SP, ARG, h, vp(pairs), 0)
    expect(SP, ARG, h, vp(pairs), FRAMES + 1)              # beyond max_frames
    expect(SP, STATE, h, vp(pairs), 1)                     # not the configured frame count
    expect(SP, ARG, h, vp(np.array([[0, 3], [1, 2]], np.int32)), 2)   # index outside the table
    expect(SP, ARG, h, vp(np.array([[0, 1], [-1, 2]], np.int32)), 2)
    expect(RUN, STATE, h)                                  # the refused calls set nothing
    for i in range(3):
        ctx.batch_upload_image(i, img)
    expect(SP, OK, h, vp(pairs), 2)
    expect(RUN, STATE, h)                                  # images uploaded, pyramids not built
    ctx.batch_run(_lib.STAGE_PYRAMID)
    ctx.batch_set_points(0, pts[:8])
    ctx.batch_set_points(1, pts[:0])
    expect(RUN, ARG, None)
    expect(RUN, OK, h)
    expect(GET, ARG, None, 0, O, S, E, 4)
    expect(GET, ARG, h, -1, O, S, E, 4)
    expect(GET, ARG, h, FRAMES, O, S, E, 4)                # frame beyond max_frames
    expect(GET, ARG, h, 0, O, S, E, -1)
    expect(GET, ARG, h, 0, O, S, E, CAP + 1)
    expect(GET, OK, h, 0, O, S, E, 8)
    expect(GET, OK, h, 1, None, None, None, 0)
    ctx.batch_configure(3, W, H, 1)                        # another table: the pairs are gone
    expect(RUN, STATE, h)

    # ---- inside the lock-step loop ----
    ctx.seq_configure(1, W, H)
    expect(T, STATE, h, I, I, W, H, W, P, 4, O, S, E)
    expect(F, STATE, h, I, I, W, H, W, P, 4, O, S, E, K, pn)
    expect(SP, STATE, h, vp(pairs[:1]), 1)
    expect(RUN, STATE, h)
    expect(GET, STATE, h, 0, O, S, E, 4)
    ctx.batch_configure(4, W, H, 1)                        # leaves the loop
    expect(T, OK, h, I, I, W, H, W, P, 4, O, S, E)
    return s.report()


if __name__ == "__main__":
    sys.exit(main())
