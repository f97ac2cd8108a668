"""Argument sweep over the four calls of include/vo_flow_flags.h: flags with a bit other than 4 and 8, windows without a kernel, NULL
pointers, n < 0, n > capacity, sizes beyond the context's, short strides, calls in the wrong state (the throughput mode's included).
Every such call must come back with the documented code -- never a fault, never a silent success -- and leave vo_last_error filled;
a refused call writes nothing.  Run as a SCRIPT in a child process by tests/test_gpu_flow_flags.py (a fault would otherwise take the
test session down with it); prints one JSON object {"checked": n, "covered": [...], "failures": [...]} and exits 0 iff there is no
failure.  Needs a GPU (vo_create)."""
import sys

import numpy as np

from flow_sweep_common import ARG, CAP, FRAMES, OK, SENT, STATE, H, W, Sweep, _lib, vp

BAD_FLAGS = (1, 2, 3, 5, 16, 20, 0x100, -1, -4)
BAD_WINDOWS = (-1, 0, 4, 6, 22, 23)
GUESS, EIG = _lib.FLAG_USE_INITIAL_FLOW, _lib.FLAG_GET_MIN_EIGENVALS


def main():
    s = Sweep()
    lib, ctx, h, fails, expect, untouched = s.lib, s.ctx, s.h, s.fails, s.expect, s.untouched
    img, pts, out, st, err, pn = s.img, s.pts, s.out, s.st, s.err, s.pn
    I, P, O, S, E, K = s.pointers
    T, F, RUN, SET = "voflag_track", "voflag_feature_tracking", "voflag_batch_run", "voflag_batch_set_guess"

    # ---- flags and windows without a kernel: refused before anything else happens ----
    for fl in BAD_FLAGS:
        expect(T, ARG, h, I, I, W, H, W, P, 4, 15, fl, O, S, E)
        expect(F, ARG, h, I, I, W, H, W, P, 4, 15, fl, O, S, E, K, pn)
    for win in BAD_WINDOWS:
        expect(T, ARG, h, I, I, W, H, W, P, 4, win, GUESS, O, S, E)
        expect(F, ARG, h, I, I, W, H, W, P, 4, win, EIG, O, S, E, K, pn)
    untouched("a call with flags or a window that have no kernel")

    # ---- voflag_track ----
    expect(T, ARG, None, I, I, W, H, W, P, 4, 15, GUESS, O, S, E)
    expect(T, ARG, h, None, I, W, H, W, P, 4, 15, GUESS, O, S, E)
    expect(T, ARG, h, I, None, W, H, W, P, 4, 15, GUESS, O, S, E)
    expect(T, ARG, h, I, I, W, H, W, None, 4, 15, GUESS, O, S, E)
    expect(T, ARG, h, I, I, W, H, W, P, 4, 15, GUESS, None, S, E)
    expect(T, ARG, h, I, I, W, H, W, P, 4, 15, EIG, O, None, E)
    expect(T, ARG, h, I, I, W, H, W, P, -1, 15, GUESS, O, S, E)
    expect(T, ARG, h, I, I, W, H, W, P, CAP + 1, 15, GUESS, O, S, E)
    expect(T, ARG, h, I, I, W + 8, H, W + 8, P, 4, 15, GUESS, O, S, E)
    expect(T, ARG, h, I, I, W, H + 8, W, P, 4, 15, EIG, O, S, E)
    expect(T, ARG, h, I, I, 16, H, W, P, 4, 15, GUESS, O, S, E)
    expect(T, ARG, h, I, I, W, H, W - 1, P, 4, 15, GUESS | EIG, O, S, E)
    expect(T, OK, h, I, I, W, H, W, P, 0, 15, GUESS, O, S, E)          # n == 0: VO_OK, nothing written
    expect(T, OK, h, I, I, W, H, W, None, 0, 5, EIG, None, None, None)
    untouched("a refused / empty voflag_track call")

    # ---- voflag_feature_tracking ----
    expect(F, ARG, None, I, I, W, H, W, P, 4, 7, GUESS, O, S, E, K, pn)
    expect(F, ARG, h, None, I, W, H, W, P, 4, 7, GUESS, O, S, E, K, pn)
    expect(F, ARG, h, I, I, W, H, W, None, 4, 7, GUESS, O, S, E, K, pn)
    expect(F, ARG, h, I, I, W, H, W, P, 4, 7, GUESS, None, S, E, K, pn)
    expect(F, ARG, h, I, I, W, H, W, P, 4, 7, EIG, O, None, E, K, pn)
    expect(F, ARG, h, I, I, W, H, W, P, 4, 7, GUESS, O, S, E, K, None)
    expect(F, ARG, h, I, I, W, H, W, P, -1, 7, GUESS, O, S, E, K, pn)
    expect(F, ARG, h, I, I, W, H, W, P, CAP + 1, 7, GUESS, O, S, E, K, pn)
    expect(F, ARG, h, I, I, W, H, W - 1, P, 4, 7, EIG, O, S, E, K, pn)
    expect(F, OK, h, I, I, W, H, W, P, 0, 7, GUESS, O, S, E, K, pn)
    untouched("a refused / empty voflag_feature_tracking call")

    # ---- the good calls: every flag value, every window, the optional outputs, the capacity ----
    out[:] = 41.0   # guesses
    for fl in (0, GUESS, EIG, GUESS | EIG):
        expect(T, OK, h, I, I, W, H, W, P, 4, 15, fl, O, S, E)
    for win in (5, 7, 9, 11, 13, 17, 19, 21):
        expect(T, OK, h, I, I, W, H, W, P, 4, win, GUESS | EIG, O, S, E)
    expect(T, OK, h, I, I, W, H, W, P, 4, 15, EIG, O, S, None)          # err is optional
    out[:] = SENT
    st[:] = 9
    err[:] = SENT
    expect(T, OK, h, I, I, W, H, W, P, CAP, 15, GUESS | EIG, O, S, E)   # n == max_pts is allowed
    if (out[CAP:] != SENT).any() or (st[CAP:] != 9).any() or (err[CAP:] != SENT).any():
        fails.append("voflag_track wrote beyond n")
    expect(F, OK, h, I, I, W, H, W, vp(pts.copy()), 4, 7, GUESS, O, S, None, None, pn)   # err and keep_idx are optional

    # ---- throughput mode ----
    pairs = np.array([[0, 1], [1, 2]], np.int32)
    fresh = _lib.Context(0, W, H, CAP, FRAMES)
    expect(RUN, STATE, fresh.h, 15, GUESS)                 # no table configured
    expect(SET, STATE, fresh.h, 0, P, 4)
    fresh.close()
    ctx.batch_configure(3, W, H, 2)
    expect(RUN, STATE, h, 15, EIG)                         # configured, no pairs
    expect(SET, STATE, h, 0, P, 4)
    expect(RUN, ARG, None, 15, GUESS)
    expect(SET, ARG, None, 0, P, 4)
    for i in range(3):
        ctx.batch_upload_image(i, img)
    ctx.flow_batch_set_pairs(pairs)
    expect(RUN, STATE, h, 15, EIG)                         # images uploaded, pyramids not built
    ctx.batch_run(_lib.STAGE_PYRAMID)
    ctx.batch_set_points(0, pts[:8])
    ctx.batch_set_points(1, pts[:0])
    for fl in BAD_FLAGS:
        expect(RUN, ARG, h, 15, fl)
    for win in BAD_WINDOWS:
        expect(RUN, ARG, h, win, GUESS)
    expect(SET, ARG, h, -1, P, 4)
    expect(SET, ARG, h, 2, P, 4)                           # frame outside the configured frames
    expect(SET, ARG, h, 0, P, -1)
    expect(SET, ARG, h, 0, P, CAP + 1)
    expect(SET, ARG, h, 0, None, 4)
    expect(RUN, STATE, h, 15, GUESS)                       # no guess, no run since the pairs were set
    expect(SET, OK, h, 0, P, 8)
    expect(RUN, STATE, h, 15, GUESS | EIG)                 # frame 1 has none yet
    expect(SET, OK, h, 1, None, 0)                         # (a frame without points: n == 0, no array needed)
    expect(RUN, OK, h, 15, GUESS)
    expect(RUN, OK, h, 21, GUESS | EIG)                    # the previous run's results are the guesses
    expect(RUN, OK, h, 9, EIG)
    expect(RUN, OK, h, 15, 0)
    if lib.voflow_batch_get(h, 0, O, S, E, 8) != OK:
        fails.append("voflow_batch_get after voflag_batch_run")
    ctx.flow_batch_set_pairs(pairs)                        # pairs set again: the rows count as unwritten
    expect(RUN, STATE, h, 15, GUESS)
    expect(RUN, OK, h, 15, EIG)                            # ... a run without the flag writes them
    expect(RUN, OK, h, 15, GUESS)
    ctx.batch_configure(3, W, H, 1)                        # another table: the pairs are gone
    expect(RUN, STATE, h, 15, EIG)
    expect(SET, STATE, h, 0, P, 4)

    # ---- inside the lock-step loop ----
    ctx.seq_configure(1, W, H)
    expect(T, STATE, h, I, I, W, H, W, P, 4, 15, GUESS, O, S, E)
    expect(F, STATE, h, I, I, W, H, W, P, 4, 7, EIG, O, S, E, K, pn)
    expect(RUN, STATE, h, 15, GUESS)
    expect(SET, STATE, h, 0, P, 4)
    ctx.batch_configure(4, W, H, 1)                        # leaves the loop
    expect(T, OK, h, I, I, W, H, W, P, 4, 15, GUESS, O, S, E)
    return s.report()


if __name__ == "__main__":
    sys.exit(main())
