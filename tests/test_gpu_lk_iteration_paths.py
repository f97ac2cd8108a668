"""The cases of tests/test_lk_iteration_paths.py on the MI355X: every case a frame of one batch through the C ABI (lk_circular_kernel),
one launch per (max_count, epsilon), and the border case through voflow_track for the err kernels (lk_flow_kernel).  Status on every
hop, positions as raw bits on every hop the checker reports alive, err bit for bit where the checker's status is 1."""
import numpy as np
import pytest

import lk_iteration_cases as ic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(volib):
    c = volib.Context(0, ic.W, ic.H, 64, len(ic.CASES))
    yield c
    c.close()


def test_the_sweep_takes_every_exit(orc):
    ic.premises(orc)


@pytest.mark.parametrize("eps", ic.EPSILONS)
@pytest.mark.parametrize("max_count", ic.MAX_COUNTS)
def test_batch_chain_equals_checker(ctx, volib, orc, max_count, eps):
    cases = [ic.case(name) for name in ic.CASES]
    nf = len(cases)
    ctx.set_params(lk_full_chain=1, lk_max_level=ic.MAX_LEVEL, lk_max_count=max_count, lk_epsilon=eps)
    try:
        ctx.batch_configure(4 * nf, ic.W, ic.H, nf)
        for f, c in enumerate(cases):
            for i, im in enumerate(c["imgs"]):
                ctx.batch_upload_image(4 * f + i, im)
        ctx.batch_set_quads(np.arange(4 * nf, dtype=np.int32).reshape(nf, 4))
        for f, c in enumerate(cases):
            ctx.batch_set_points(f, c["pts"])
        ctx.batch_run(volib.STAGE_PYRAMID | volib.STAGE_LK)
        ctx.batch_sync()
        for f, (name, c) in enumerate(zip(ic.CASES, cases)):
            g = ctx.batch_get_tracks(f, len(c["pts"]))
            trk = np.stack([g[k] for k in ("r0", "r1", "l1", "l0_ret")])
            ic.assert_chain(trk, g["status4"], ic.oracle(orc, name, max_count, eps), (name, max_count, eps))
    finally:
        ctx.set_params(lk_full_chain=0, lk_max_level=3, lk_max_count=30, lk_epsilon=0.01)


def test_two_image_call_equals_checker(ctx, orc):
    """voflow_track (lk_flow_kernel: the body with the err epilogue) on the border case, the whole sweep"""
    c = ic.case("borders")
    lost = 0
    try:
        for mc in ic.MAX_COUNTS:
            for eps in ic.EPSILONS:
                ctx.set_params(lk_max_level=ic.MAX_LEVEL, lk_max_count=mc, lk_epsilon=eps)
                nxt, st, err = ctx.flow_track(c["imgs"][ic.FLOW_PAIR[0]], c["imgs"][ic.FLOW_PAIR[1]], c["pts"])
                wn, ws, we = ic.oracle_flow(orc, "borders", mc, eps)
                assert np.array_equal(st, ws), (mc, eps, "status")
                alive = ws == 1
                assert alive.any()
                lost += int((~alive).sum())
                assert (ic.bits(nxt) == ic.bits(wn)).all(-1)[alive].all(), (mc, eps, "positions")
                assert np.array_equal(ic.bits(err)[alive], ic.bits(we)[alive]), (mc, eps, "err")
        assert lost > 0, "no window of the sweep left the image"
    finally:
        ctx.set_params(lk_max_level=3, lk_max_count=30, lk_epsilon=0.01)
