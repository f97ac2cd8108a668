"""lk_circular_queue_kernel on the MI355X: batches of 16, 17 and 24 frames of 96 x 88 images go through the per-XCD ticket queues
(launch_lk_circular: 16 frames and more), the same frames in batches of 8 through the static lk_circular_kernel.  The frames of one
XCD (f & 7 == HEAVY) carry 64 points and every other frame 1, so the heavy XCD's queue is the one that other XCDs' surplus
workgroups find tickets in; one batch has an empty frame.  Raw per-hop tracks and status, read the way
tests/test_gpu_lk_level_setup.py reads them, equal bit for bit; every batch is launched twice, on the two counter sets."""
import numpy as np
import pytest

import lk_queue_cases as qc

pytestmark = pytest.mark.gpu

HEAVY = 5
FRAMES = 24


def counts(n_frames, empty=None):
    c = [64 if f & 7 == HEAVY else 1 for f in range(n_frames)]
    if empty is not None:
        c[empty] = 0
    return c


@pytest.fixture(scope="module")
def ctx(volib):
    c = volib.Context(0, qc.W, qc.H, qc.N, FRAMES)
    c.set_params(lk_full_chain=0, lk_max_level=3, lk_max_count=30, lk_min_eig_threshold=0.001)
    yield c
    c.close()


def run_batch(ctx, volib, frames, cnt, launches=1):
    """frames: the frame numbers of the batch (their images, points and quads are those of lk_queue_cases); `launches` results,
    each a list of (trk [4, c, 2], status [4, c]) per frame"""
    nf = len(frames)
    imgs, pts = qc.images(), qc.points(FRAMES)
    ctx.batch_configure(4, qc.W, qc.H, nf)
    for i, im in enumerate(imgs):
        ctx.batch_upload_image(i, im)
    ctx.batch_set_quads(qc.quads(FRAMES)[list(frames)])
    for k, f in enumerate(frames):
        ctx.batch_set_points(k, pts[f][:cnt[f]])
    out = []
    for n in range(launches):
        ctx.batch_run(volib.STAGE_PYRAMID | volib.STAGE_LK if n == 0 else volib.STAGE_LK)
        ctx.batch_sync()
        res = []
        for k, f in enumerate(frames):
            if cnt[f] == 0:
                res.append((np.zeros((4, 0, 2), np.float32), np.zeros((4, 0), np.uint8)))
                continue
            g = ctx.batch_get_tracks(k, cnt[f])
            res.append((np.stack([g[key] for key in ("r0", "r1", "l1", "l0_ret")]).copy(), g["status4"].copy()))
        out.append(res)
    return out


_STATIC = {}


def static_frames(ctx, volib, cnt):
    """every frame through lk_circular_kernel: batches of 8 (fewer than 16 frames never take the queues), once per set of counts"""
    key = tuple(cnt)
    if key not in _STATIC:
        res = []
        for first in range(0, len(cnt), 8):
            frames = list(range(first, min(first + 8, len(cnt))))
            res += run_batch(ctx, volib, frames, cnt)[0]
        _STATIC[key] = res
    return _STATIC[key]


def assert_same(got, want, what):
    for f, ((gt, gs), (wt, ws)) in enumerate(zip(got, want)):
        assert np.array_equal(gs, ws), (what, f, "status")
        assert np.array_equal(gt.view(np.uint32), wt.view(np.uint32)), (what, f, "positions")


@pytest.mark.parametrize("n_frames,empty", [(16, None), (17, None), (24, None), (24, 2)], ids=["16", "17", "24", "24-empty-frame"])
def test_queue_batches_equal_static_batches(ctx, volib, n_frames, empty):
    cnt = counts(FRAMES, empty)
    want = static_frames(ctx, volib, cnt)[:n_frames]
    heavy = want[HEAVY][1]
    assert heavy.shape == (4, 64) and (heavy[3] == 1).sum() >= 20 and (heavy[0] == 0).any()   # tracked and lost points
    first, second = run_batch(ctx, volib, list(range(n_frames)), cnt, launches=2)
    assert_same(first, want, (n_frames, "first launch"))
    assert_same(second, want, (n_frames, "second launch: the other counter set"))
