"""Argument sweep over the four calls of include/vo_flow_win.h: windows without a kernel, NULL pointers, n < 0, n > capacity, sizes
beyond the context's, short strides, calls in the wrong state.  Every such call must come back with the documented code -- never a
fault, never a silent success -- and leave vo_last_error filled; a refused call writes nothing.  Run as a SCRIPT in a child process
by tests/test_gpu_flow_win.py (a fault would otherwise take the test session down with it); prints one JSON object
{"checked": n, "covered": [...], "failures": [...]} and exits 0 iff there is no failure.  Needs a GPU (vo_create)."""
import ctypes as C
import sys

import numpy as np

from flow_sweep_common import ARG, CAP, FRAMES, OK, SENT, STATE, H, W, Sweep, _lib, vp

BAD_WINDOWS = (-1, 0, 3, 4, 6, 20, 22, 23, 31)


def main():
    s = Sweep(no_message=("vowin_max_level",))
    lib, ctx, h, fails, expect, untouched = s.lib, s.ctx, s.h, s.fails, s.expect, s.untouched
    img, pts, out, st, err, pn = s.img, s.pts, s.out, s.st, s.err, s.pn
    I, P, O, S, E, K = s.pointers
    T, F, RUN, ML = "vowin_track", "vowin_feature_tracking", "vowin_batch_run", "vowin_max_level"

    # ---- windows without a kernel: refused before anything else happens ----
    for win in BAD_WINDOWS:
        expect(T, ARG, h, I, I, W, H, W, P, 4, win, O, S, E)
        expect(F, ARG, h, I, I, W, H, W, P, 4, win, O, S, E, K, pn)
    untouched("a call with a window that has no kernel")

    # ---- vowin_track ----
    expect(T, ARG, None, I, I, W, H, W, P, 4, 15, O, S, E)
    expect(T, ARG, h, None, I, W, H, W, P, 4, 15, O, S, E)
    expect(T, ARG, h, I, None, W, H, W, P, 4, 15, O, S, E)
    expect(T, ARG, h, I, I, W, H, W, None, 4, 15, O, S, E)
    expect(T, ARG, h, I, I, W, H, W, P, 4, 15, None, S, E)
    expect(T, ARG, h, I, I, W, H, W, P, 4, 15, O, None, E)
    expect(T, ARG, h, I, I, W, H, W, P, -1, 15, O, S, E)
    expect(T, ARG, h, I, I, W, H, W, P, CAP + 1, 15, O, S, E)
    expect(T, ARG, h, I, I, W + 8, H, W + 8, P, 4, 15, O, S, E)
    expect(T, ARG, h, I, I, W, H + 8, W, P, 4, 15, O, S, E)
    expect(T, ARG, h, I, I, 16, H, W, P, 4, 15, O, S, E)
    expect(T, ARG, h, I, I, W, H, W - 1, P, 4, 15, O, S, E)
    expect(T, OK, h, I, I, W, H, W, P, 0, 15, O, S, E)          # n == 0: VO_OK, nothing written
    expect(T, OK, h, I, I, W, H, W, None, 0, 5, None, None, None)
    untouched("a refused / empty vowin_track call")
    ctx.set_params(input_format=_lib.FMT_BGR8)
    expect(T, ARG, h, I, I, 100, H, 299, P, 4, 15, O, S, E)     # stride below 3 bytes per pixel
    ctx.set_params(input_format=_lib.FMT_GRAY8)

    # ---- vowin_feature_tracking ----
    expect(F, ARG, None, I, I, W, H, W, P, 4, 7, O, S, E, K, pn)
    expect(F, ARG, h, None, I, W, H, W, P, 4, 7, O, S, E, K, pn)
    expect(F, ARG, h, I, None, W, H, W, P, 4, 7, O, S, E, K, pn)
    expect(F, ARG, h, I, I, W, H, W, None, 4, 7, O, S, E, K, pn)
    expect(F, ARG, h, I, I, W, H, W, P, 4, 7, None, S, E, K, pn)
    expect(F, ARG, h, I, I, W, H, W, P, 4, 7, O, None, E, K, pn)
    expect(F, ARG, h, I, I, W, H, W, P, 4, 7, O, S, E, K, None)
    expect(F, ARG, h, I, I, W, H, W, P, -1, 7, O, S, E, K, pn)
    expect(F, ARG, h, I, I, W, H, W, P, CAP + 1, 7, O, S, E, K, pn)
    expect(F, ARG, h, I, I, W + 8, H, W + 8, P, 4, 7, O, S, E, K, pn)
    expect(F, ARG, h, I, I, W, H, W - 1, P, 4, 7, O, S, E, K, pn)
    expect(F, OK, h, I, I, W, H, W, P, 0, 7, O, S, E, K, pn)
    untouched("a refused / empty vowin_feature_tracking call")

    # ---- the good calls: every window, the optional outputs, the capacity ----
    for win in (5, 7, 9, 11, 13, 15, 17, 19, 21):
        expect(T, OK, h, I, I, W, H, W, P, 4, win, O, S, E)
    expect(T, OK, h, I, I, W, H, W, P, 4, 15, O, S, None)        # err is optional
    expect(T, OK, h, I, I, W, H, W, P, CAP, 15, O, S, E)         # n == max_pts is allowed
    if (out[CAP:] != SENT).any() or (st[CAP:] != 9).any() or (err[CAP:] != SENT).any():
        fails.append("vowin_track wrote beyond n")
    expect(F, OK, h, I, I, W, H, W, vp(pts.copy()), 4, 7, O, S, None, None, pn)   # err and keep_idx are optional

    # ---- vowin_max_level ----
    lvl = C.c_int(-9)
    pl = C.addressof(lvl)
    expect(ML, ARG, None, W, H, pl)
    expect(ML, ARG, h, W, H, None)
    expect(ML, ARG, h, 16, H, pl)
    expect(ML, ARG, h, W, 16, pl)
    expect(ML, ARG, h, W + 1, H, pl)
    expect(ML, ARG, h, W, H + 1, pl)
    if lvl.value != -9:
        fails.append("a refused vowin_max_level call wrote its output")
    expect(ML, OK, h, W, H, pl)
    if lvl.value != 2:   # 320 x 96 -> 160 x 48 -> 80 x 24 -> (40 x 12: not larger than 21)
        fails.append("vowin_max_level(320, 96) = %d, expected 2" % lvl.value)

    # ---- throughput mode ----
    pairs = np.array([[0, 1], [1, 2]], np.int32)
    fresh = _lib.Context(0, W, H, CAP, FRAMES)
    expect(RUN, STATE, fresh.h, 15)                        # no table configured
    fresh.close()
    ctx.batch_configure(3, W, H, 2)
    expect(RUN, STATE, h, 15)                              # configured, no pairs
    expect(RUN, ARG, None, 15)
    for i in range(3):
        ctx.batch_upload_image(i, img)
    ctx.flow_batch_set_pairs(pairs)
    expect(RUN, STATE, h, 15)                              # images uploaded, pyramids not built
    ctx.batch_run(_lib.STAGE_PYRAMID)
    ctx.batch_set_points(0, pts[:8])
    ctx.batch_set_points(1, pts[:0])
    for win in BAD_WINDOWS:
        expect(RUN, ARG, h, win)
    expect(RUN, OK, h, 15)
    expect(RUN, OK, h, 21)
    if lib.voflow_batch_get(h, 0, O, S, E, 8) != OK:
        fails.append("voflow_batch_get after vowin_batch_run")
    ctx.batch_configure(3, W, H, 1)                        # another table: the pairs are gone
    expect(RUN, STATE, h, 15)

    # ---- inside the lock-step loop ----
    ctx.seq_configure(1, W, H)
    expect(T, STATE, h, I, I, W, H, W, P, 4, 15, O, S, E)
    expect(F, STATE, h, I, I, W, H, W, P, 4, 7, O, S, E, K, pn)
    expect(RUN, STATE, h, 15)
    expect(ML, OK, h, W, H, pl)                            # (no GPU work, no state)
    ctx.batch_configure(4, W, H, 1)                        # leaves the loop
    expect(T, OK, h, I, I, W, H, W, P, 4, 15, O, S, E)
    return s.report()


if __name__ == "__main__":
    sys.exit(main())
