"""The two-image tracker with flags of include/vo_flow_flags.h on the MI355X: voflag_track, voflag_feature_tracking,
voflag_batch_set_guess and voflag_batch_run.  The expected side of every comparison is the checker's (tests/flow_flags_cases.py):
for USE_INITIAL_FLOW its own level loop started at the guess, for GET_MIN_EIGENVALS the checker without an err vector and its
threshold as a bracket around every value -- positions, status and err BIT FOR BIT, every point, after the premises that make a
guess-ignoring or epilogue-keeping implementation fail.  Also: flags 0 is the vowin_* call, the calls leave the rest of the
context alone, and an argument sweep in a child process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import flow_cases as fc
import flow_flags_cases as gc
import flow_win_cases as wc
from test_gpu_flow import _batch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def ctx(gpu_ctx):
    """the shared context with the default LK depth, iteration count and gray input, before and after"""
    gpu_ctx.set_params(lk_max_level=3, lk_max_count=30, input_format=0)
    yield gpu_ctx
    gpu_ctx.set_params(lk_max_level=3, lk_max_count=30, input_format=0)


def _track(ctx, c, **kw):
    ctx.set_params(lk_max_level=c["lk_max_level"], lk_max_count=c.get("max_count", 30))
    h, w = c["prev"].shape
    assert ctx.flow_max_level(w, h) == c["max_level"]
    return ctx.flow_track(c["prev"], c["next"], c["pts"], win=c["win"], **kw)


# ---- USE_INITIAL_FLOW ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["crop", "lattice", "L0-L1"])
@pytest.mark.parametrize("win", [7, 15, 21])
def test_guess_equal_prev_gives_the_flags_0_bytes(ctx, orc, small_seq, win, name):
    c = wc.case(name, win, small_seq, orc)
    plain = _track(ctx, c)
    fc.assert_same(plain, c["want"], (name, win, "flags 0"))
    got = _track(ctx, c, guess=c["pts"])
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got, plain)), (name, win)


@pytest.mark.parametrize("win,level", [(21, 0), (21, 3), (15, 0), (7, 3)])
def test_guess_is_the_answer(ctx, orc, small_seq, win, level):
    c = gc.guess_case("answer", win, level, small_seq, orc)
    gc.guess_premises(c, "answer")
    fc.assert_same(_track(ctx, c, guess=c["guess"]), c["want"], ("answer", win, level))


@pytest.mark.parametrize("win", [7, 15, 21])
def test_random_guess(ctx, orc, small_seq, win):
    c = gc.guess_case("random", win, 3, small_seq, orc)
    gc.guess_premises(c, "random")
    fc.assert_same(_track(ctx, c, guess=c["guess"]), c["want"], ("random", win))


@pytest.mark.parametrize("win", [7, 15, 21])
def test_adversarial_guesses(ctx, orc, small_seq, win):
    c = gc.adversarial_case(win, small_seq, orc)
    gc.adversarial_premises(c)
    fc.assert_same(_track(ctx, c, guess=c["guess"]), c["want"], ("adversarial", win))


# ---- GET_MIN_EIGENVALS --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["crop60", "pts596", "lattice", "flat"])
@pytest.mark.parametrize("win", [21, 9])
def test_min_eigenvalues_by_bracketing(ctx, orc, small_seq, win, name):
    s = gc.eig_set(name, win, small_seq, orc)
    c = dict(prev=s["img"], next=s["img"], pts=s["pts"], win=win, lk_max_level=0, max_level=0)
    gc.check_min_eigenvals(orc, s, _track(ctx, c, min_eigenvals=True), (name, win))


def test_min_eigenvalues_skip_the_final_check(ctx, orc, small_seq):
    c = gc.final_check_case(small_seq, orc)
    nxt, st, err = _track(ctx, c, min_eigenvals=True)
    fc.assert_same((nxt, st, None), c["want_no_err"], "lattice 2.5")
    assert (st[c["flips"]] == 1).all()
    adm = gc.admissible(c["prev"], c["pts"], 21)
    assert np.all(fc.bits(err[~adm]) == 0) and (err[adm] > 0).sum() >= 1000
    fc.assert_same(_track(ctx, c, min_eigenvals=True, want_err=False), c["want_no_err"], "lattice 2.5, err == NULL")
    fc.assert_same(_track(ctx, c), c["with_err"], "lattice 2.5, flags 0")


def test_both_flags(ctx, orc, small_seq):
    c = gc.guess_case("answer", 21, 0, small_seq, orc)
    gc.guess_premises(c, "answer")
    nxt, st, err = _track(ctx, c, guess=c["guess"], min_eigenvals=True)
    fc.assert_same((nxt, st, None), c["want_no_err"], "both flags")
    s = gc.eig_set("pts596", 21, small_seq, orc)
    bad = [i for i in range(596) if not gc._bracket(orc, s["img"], s["pts"][i], 21, err[i])]
    assert not bad, bad[:8]


# ---- the other entry points -----------------------------------------------------------------------------------------------------
def test_flags_0_is_the_win_call(ctx, orc, small_seq, volib):
    c = wc.case("L0-L1", 15, small_seq, orc)
    h, w = c["prev"].shape
    plain = ctx.flow_track(c["prev"], c["next"], c["pts"], win=15)
    out, st, err = np.full((596, 2), 5.5, np.float32), np.zeros(596, np.uint8), np.zeros(596, np.float32)
    p = lambda a: a.ctypes.data_as(volib.C.c_void_p)
    assert volib.load().voflag_track(ctx.h, p(c["prev"]), p(c["next"]), w, h, w, p(c["pts"]), 596, 15, 0, p(out), p(st), p(err)) == 0
    assert all(x.tobytes() == y.tobytes() for x, y in zip((out, st, err), plain)), "voflag_track(flags 0) gives the bytes of vowin_track"
    _batch(ctx, small_seq)
    ctx.flow_batch_run(win=15)
    counts = [596, 100, 0, 1, 64, 596]
    want = [ctx.flow_batch_get(f, n) for f, n in enumerate(counts)]
    ctx.flow_batch_run(win=7)
    assert volib.load().voflag_batch_run(ctx.h, 15, 0) == 0
    for f, n in enumerate(counts):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(ctx.flow_batch_get(f, n), want[f])), "voflag_batch_run(flags 0), frame %d" % f


def test_feature_tracking_with_a_guess(ctx, orc, small_seq):
    c = wc.case("L0-R0", 15, small_seq, orc)
    guess = (c["pts"] + np.random.default_rng(7).uniform(-6, 6, c["pts"].shape)).astype(np.float32)
    nxt, st, err = gc.driver(c["prev"], c["next"], c["pts"], guess, win=15, max_level=c["max_level"])
    assert (fc.bits(nxt) != fc.bits(c["want"][0])).any(1).sum() >= 500, "the guess matters"
    w0, w1, wst, wkeep = fc.delete_unmatch_features(c["pts"], nxt, st)
    assert 0 < len(wkeep) < (st == 1).sum() < len(st)
    r = ctx.feature_tracking(c["prev"], c["next"], c["pts"], win=15, guess=guess)
    assert r["n_out"] == len(wkeep) and np.array_equal(r["keep_idx"], wkeep) and np.array_equal(r["status"], wst)
    assert np.array_equal(fc.bits(r["points0"]), fc.bits(w0)) and np.array_equal(fc.bits(r["points1"]), fc.bits(w1))
    assert np.array_equal(fc.bits(r["err"]), fc.bits(err)), "err is not compacted"


def test_batch_with_guesses_frame_by_frame(ctx, orc, small_seq, volib):
    imgs, pairs, counts, pts = _batch(ctx, small_seq)
    with pytest.raises(volib.VoError) as e:   # nothing in the next-position rows yet
        ctx.flow_batch_run(win=15, guess=True)
    assert e.value.code == volib.VO_ERR_STATE
    rng = np.random.default_rng(11)
    guesses = [(pts[:n] + rng.uniform(-5, 5, (n, 2))).astype(np.float32) for n in counts]
    for f, g in enumerate(guesses[:-1]):
        ctx.flow_batch_set_guess(f, g)
    with pytest.raises(volib.VoError) as e:   # one frame still without a guess
        ctx.flow_batch_run(win=15, guess=True)
    assert e.value.code == volib.VO_ERR_STATE
    ctx.flow_batch_set_guess(5, guesses[5])
    ctx.flow_batch_run(win=15, guess=True)
    first = [ctx.flow_batch_get(f, n) for f, n in enumerate(counts)]
    ctx.flow_batch_run(win=15, guess=True)   # no new guess: starts from the first run's results
    second = [ctx.flow_batch_get(f, n) for f, n in enumerate(counts)]
    differ = 0
    for f, ((a, b), n) in enumerate(zip(pairs, counts)):
        if not n:
            continue
        want = gc.driver(imgs[a], imgs[b], pts[:n], guesses[f], win=15, max_level=2)
        fc.assert_same(first[f], want, "frame %d" % f)
        again = gc.driver(imgs[a], imgs[b], pts[:n], want[0], win=15, max_level=2)
        fc.assert_same(second[f], again, "second run, frame %d" % f)
        differ += int((fc.bits(want[0]) != fc.bits(orc.calc_optical_flow_pyr_lk(imgs[a], imgs[b], pts[:n], win=15, max_level=2)[0])).any(1).sum())
    assert differ >= 800 and (first[0][1] == 1).sum() >= 400, "the guesses matter"
    ctx.flow_batch_run(win=15, min_eigenvals=True)
    eig = ctx.flow_batch_get(0, 596)
    fc.assert_same((eig[0], eig[1], None), gc.plain_no_err(orc, imgs[0], imgs[1], pts, win=15, max_level=2), "batch, min eigenvalues")
    assert (eig[2] > 0).sum() >= 590


def test_track_variants_of_one_call(ctx, orc, small_seq, volib):
    """a padded-stride ROI view and a BGR image of the same gray values are the contiguous gray call, with both flags at W = 9"""
    c = dict(gc.guess_case("random", 9, 3, small_seq, orc))
    h, w = c["prev"].shape
    want = ctx.flow_track(c["prev"], c["next"], c["pts"], win=9, guess=c["guess"], min_eigenvals=True)
    fc.assert_same((want[0], want[1], None), c["want_no_err"], "both flags, W = 9")
    big = np.full((2, h + 9, w + 37), 200, np.uint8)
    big[0, 4:4 + h, 11:11 + w] = c["prev"]
    big[1, 4:4 + h, 11:11 + w] = c["next"]
    roi = ctx.flow_track(big[0, 4:4 + h, 11:11 + w], big[1, 4:4 + h, 11:11 + w], c["pts"], win=9, guess=c["guess"], min_eigenvals=True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(roi, want)), "ROI view"
    ctx.set_params(input_format=volib.FMT_BGR8)
    bgr = ctx.flow_track(np.repeat(c["prev"][..., None], 3, 2), np.repeat(c["next"][..., None], 3, 2), c["pts"], win=9, guess=c["guess"], min_eigenvals=True)
    ctx.set_params(input_format=volib.FMT_GRAY8)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(bgr, want)), "BGR8"


def test_flagged_calls_leave_the_other_calls_alone(ctx, orc, small_seq):
    L, R, pts = small_seq["L"], small_seq["R"], small_seq["pts"][0]
    c = fc.case("L0-L1", small_seq, orc)
    c9 = wc.case("L0-L1", 9, small_seq, orc)
    flow_before = ctx.flow_track(c["prev"], c["next"], c["pts"])
    win_before = ctx.flow_track(c["prev"], c["next"], c["pts"], win=9)
    circ_before = {k: np.array(v) for k, v in ctx.circular_match(L[0], R[0], L[1], R[1], pts).items()}
    assert circ_before["n_out"] > 100
    g = gc.guess_case("random", 21, 3, small_seq, orc)["guess"]
    ctx.flow_track(c["prev"], c["next"], c["pts"], guess=g)
    assert ctx.kept_pair_id() == 0, "no kept pair after a flagged call"
    ctx.flow_track(c["prev"], c["next"], c["pts"], win=13, min_eigenvals=True)
    ctx.feature_tracking(L[0], R[0], pts, win=9, guess=g, min_eigenvals=True)
    assert ctx.kept_pair_id() == 0
    _batch(ctx, small_seq)
    ctx.flow_batch_run(win=11, min_eigenvals=True)
    ctx.flow_batch_run(win=11, guess=True)
    ctx.batch_sync()
    flow_after = ctx.flow_track(c["prev"], c["next"], c["pts"])
    win_after = ctx.flow_track(c["prev"], c["next"], c["pts"], win=9)
    circ_after = ctx.circular_match(L[0], R[0], L[1], R[1], pts)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(flow_before, flow_after))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(win_before, win_after))
    assert all(np.asarray(circ_before[k]).tobytes() == np.asarray(circ_after[k]).tobytes() for k in circ_before)
    fc.assert_same(flow_after, c["want"], "voflow_track after flagged calls")
    fc.assert_same(win_after, c9["want"], "vowin_track(9) after flagged calls")


def test_argument_sweep_of_the_flag_calls():
    """tests/flow_flags_sweep.py in a child process (a fault must fail THIS test, not end the session)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "flow_flags_sweep.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode in (0, 1), "flow_flags_sweep died (rc %d): %s" % (r.returncode, r.stderr[-2000:])
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    assert not rep["failures"], rep["failures"]
    assert rep["checked"] >= 40
    from visual_odom_amd import _lib
    assert sorted(rep["covered"]) == sorted(_lib.FLAG_EXPORTS)
