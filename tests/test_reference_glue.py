"""oracle/_ref: the reference's own src/feature.cpp, bucket.cpp, visualOdometry.cpp and utils.cpp, compiled where they
lie against a stand-in for the OpenCV declarations (oracle/ref_shim), with the OpenCV algorithms forwarding to the
oracle's restatement.  These tests pin the oracle's RESTATED glue (oracle/orc_glue.c: call order of the four LK hops,
deleteUnmatchFeaturesCircle's erase / age semantics, Bucket::add_feature, bucketingFeatures' aliased indexing and
duplicate emission, appendNewFeatures) and the tests' own restatements (flow_cases.delete_unmatch_features; featureTracking and
featureDetectionGoodFeaturesToTrack as checker call + restated glue) against the real sources on identical inputs.  OpenCV's own arithmetic is
not part of what is pinned here (it is absent from the reference tree: parity of LK / FAST stays unpinned)."""
import numpy as np
import pytest

import corners_emu as ce
import flow_cases as fc


@pytest.fixture(scope="module")
def ref(orc):
    if orc.ref_lib() is None:
        pytest.skip("oracle/_ref is only buildable where /root/reference exists and was not shipped")
    return orc


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_circular_matching_restatement_equals_the_reference_source(ref, small_seq):
    s = small_seq
    args = (s["L"][0], s["R"][0], s["L"][1], s["R"][1])
    # in-image points, points at / beyond the borders (negative results, status 0), and an ages array that is
    # LONGER than the points array (quirk B3: the tail survives untouched apart from the += 1)
    border = np.array([[0, 0], [479, 159], [2.5, 80.25], [-5, 50], [100, -3], [520, 100], [240, 185], [476.2, 10.7]], np.float32)
    pts = np.vstack([s["pts"][0][:150], border]).astype(np.float32)
    rng = np.random.default_rng(2)
    for ages in (None, rng.integers(0, 12, len(pts)).astype(np.int32), rng.integers(0, 12, len(pts) + 17).astype(np.int32)):
        a = ref.circular_matching(*args, pts, ages=ages)
        b = ref.ref_circular_matching(*args, pts, ages=ages)
        assert a["n_out"] == b["n_out"] and 0 < a["n_out"] < len(pts)
        for k in ("l0", "r0", "r1", "l1", "l0_ret"):
            assert np.array_equal(bits(a[k]), bits(b[k])), k
        assert np.array_equal(a["ages"], b["ages"])


def test_circular_matching_degenerate_inputs(ref, small_seq):
    s = small_seq
    args = (s["L"][0], s["R"][0], s["L"][1], s["R"][1])
    for pts in (np.zeros((0, 2), np.float32), np.array([[-50, -50]], np.float32), s["pts"][0][:1]):
        a = ref.circular_matching(*args, pts)
        b = ref.ref_circular_matching(*args, pts)
        assert a["n_out"] == b["n_out"]
        assert np.array_equal(bits(a["l1"]), bits(b["l1"])) and np.array_equal(a["ages"], b["ages"])


@pytest.mark.parametrize("rows,cols,bucket,fpb", [(376, 1241, 37, 1), (376, 1241, 37, 6), (160, 480, 16, 2), (97, 131, 10, 3)])
def test_bucketing_restatement_equals_the_reference_source(ref, rows, cols, bucket, fpb):
    rng = np.random.default_rng(rows + fpb)
    for n, extra in ((0, 0), (40, 0), (3000, 0), (3000, 25)):
        # points inside the image (the reference indexes outside its bucket vector otherwise), many per bucket,
        # ages spanning the >= 10 cut-off, optionally more ages than points (B3)
        pts = np.c_[rng.uniform(0, cols - 1e-3, n), rng.uniform(0, rows - 1e-3, n)].astype(np.float32)
        pts[: n // 10, 0] = cols - 1 - rng.uniform(0, bucket, n // 10).astype(np.float32) * 0.99  # last column: aliased buckets
        ages = rng.integers(0, 14, n + extra).astype(np.int32)
        p1, a1 = ref.bucketing_features(rows, cols, pts, ages, bucket, fpb)
        p2, a2 = ref.ref_bucketing_features(rows, cols, pts, ages, bucket, fpb)
        assert np.array_equal(bits(p1), bits(p2)) and np.array_equal(a1, a2)


def test_append_new_features_equals_the_reference_source(ref, small_seq):
    img = small_seq["L"][0]
    rng = np.random.default_rng(4)
    carried = np.c_[rng.uniform(0, img.shape[1], 30), rng.uniform(0, img.shape[0], 30)].astype(np.float32)
    ages = rng.integers(0, 9, 30).astype(np.int32)
    p2, a2 = ref.ref_append_new_features(img, carried, ages)
    fast = ref.fast_detect(img, 20, True)
    assert len(fast) > 50
    assert np.array_equal(bits(p2), bits(np.vstack([carried, fast])))
    assert np.array_equal(a2, np.concatenate([ages, np.zeros(len(fast), np.int32)]))


def _same_deletion(ref, p0, p1, st):
    """flow_cases.delete_unmatch_features == the reference's deleteUnmatchFeatures on one input, bit for bit; returns the survivors"""
    a0, a1, ast, keep = fc.delete_unmatch_features(p0, p1, st)
    b0, b1, bst = ref.ref_delete_unmatch_features(p0, p1, st)
    assert len(b0) == len(b1) == len(a0) == len(a1) == len(keep)
    assert np.array_equal(bits(a0), bits(b0)) and np.array_equal(bits(a1), bits(b1))
    assert ast.dtype == bst.dtype == np.uint8 and len(bst) == len(st) and np.array_equal(ast, bst)
    return len(b0), bst


def test_delete_unmatch_restatement_equals_the_reference_source(ref, small_seq):
    """flow_cases.delete_unmatch_features is what every voflow_feature_tracking / vowin_feature_tracking test expects: here it
    meets the function it restates (feature.cpp:20-37)"""
    c = fc.case("L0-R0", small_seq, ref)
    nxt, st, _ = c["want"]
    left = (st == 1) & ((nxt[:, 0] < 0) | (nxt[:, 1] < 0))
    assert len(st) == 596 and left.sum() >= 1 and (st == 0).sum() >= 20, "L0-R0: a tracked point that left the image, and lost ones"
    m, out = _same_deletion(ref, c["pts"], nxt, st)
    assert m == 596 - int(((st == 0) | left).sum()) and np.all(out[left] == 0)

    nan, T, F = np.nan, 1, 0
    #        0: first  1     2 3 4: a run (lost, x < 0, y < 0)        5: -0.0      6: NaN      7 (255)   8 9: a run           10     11: last
    st = [F, T, F, T, T, T, T, 255, F, T, T, F]
    p1 = [[-3, 5], [4, 4], [7, 7], [-1, 9], [9, -0.5], [-0.0, 6], [nan, 2], [3, 3], [nan, nan], [-2, -2], [8, 1], [5, 5]]
    st, p1 = np.array(st, np.uint8), np.array(p1, np.float32)
    p0 = np.arange(24, dtype=np.float32).reshape(12, 2) + 100
    drop = (st == 0) | (p1[:, 0] < 0) | (p1[:, 1] < 0)
    assert drop.tolist() == [1, 0, 1, 1, 1, 0, 0, 0, 1, 1, 0, 1]            # first and last dropped, runs of 3 and 2
    assert st[3] == 1 and p1[3, 0] < 0 and p1[3, 1] >= 0 and st[4] == 1 and p1[4, 1] < 0 and p1[4, 0] >= 0   # status 1: x < 0; y < 0
    assert st[5] == 1 and np.signbit(p1[5, 0]) and p1[5, 0] == 0 and st[6] == 1 and np.isnan(p1[6, 0])      # -0.0 and NaN: kept
    m, out = _same_deletion(ref, p0, p1, st)
    assert m == 12 - int(drop.sum()) == 5 and out.tolist() == [0, 1, 0, 0, 0, 1, 1, 255, 0, 0, 1, 0]
    assert _same_deletion(ref, p0, p1, np.zeros(12, np.uint8))[0] == 0                                       # all dropped ...
    assert _same_deletion(ref, p0, np.full((12, 2), -1, np.float32), np.ones(12, np.uint8))[0] == 0          # ... by either rule
    assert _same_deletion(ref, p0, np.abs(np.nan_to_num(p1)), np.ones(12, np.uint8))[0] == 12                # none dropped
    assert _same_deletion(ref, p0[:0], p1[:0], st[:0])[0] == 0                                               # n = 0
    assert _same_deletion(ref, p0[:1], p1[:1], st[:1])[0] == 0 and _same_deletion(ref, p0[1:2], p1[1:2], st[1:2])[0] == 1


@pytest.mark.parametrize("name", ["L0-L1", "L0-R0"])
def test_feature_tracking_equals_the_reference_source(ref, small_seq, name):
    """featureTracking (feature.cpp:64-74) compiled where it lies == calcOpticalFlowPyrLK(21 x 21, maxLevel 3) of the checker +
    the restated deleteUnmatchFeatures: what featureTracking_hip is held to on the device"""
    c = fc.case(name, small_seq, ref)
    fc.assert_not_vacuous(name, c)
    nxt, st, _ = c["want"]
    w0, w1, wst, keep = fc.delete_unmatch_features(c["pts"], nxt, st)
    assert 500 <= len(keep) < (st == 1).sum() <= 596 - 20, "lost points, and tracked points that left the image"
    g0, g1, gst = ref.ref_feature_tracking(c["prev"], c["next"], c["pts"])
    assert len(g0) == len(g1) == len(keep) and len(gst) == 596
    assert np.array_equal(bits(g0), bits(w0)) and np.array_equal(bits(g1), bits(w1)) and np.array_equal(gst, wst)
    e0, e1, est = ref.ref_feature_tracking(c["prev"], c["next"], c["pts"][:0])
    assert len(e0) == len(e1) == len(est) == 0


def test_feature_detection_gftt_equals_the_reference_source(ref, small_seq):
    """featureDetectionGoodFeaturesToTrack (feature.cpp:49-62) compiled where it lies == corners_ref.c's cr_detect at the
    reference's literals 5000 / 0.01 / 5.0: on a frame the limit leaves alone, and on one it cuts (5 pixels apart, 480 x 160
    cannot hold 5000 corners: the noise image is 640 x 480)"""
    for img, binds in ((small_seq["L"][0], False), (ce.noise(640, 480, 21), True)):
        want, n, _ = ce.ref_detect(img, 5000, 0.01, 5.0)
        unlimited = ce.ref_detect(img, 0, 0.01, 5.0)[1]
        assert (unlimited > 5000 and n == 5000) if binds else (100 < unlimited == n < 5000), (unlimited, n)
        got, m = ref.ref_feature_detection_gftt(img)
        assert m == n == len(got) and np.array_equal(bits(got), bits(want))
        few, m = ref.ref_feature_detection_gftt(img, cap=7)
        assert m == n and np.array_equal(bits(few), bits(want[:7]))
    img = ce.noise(131, 67, 3)
    want, n, _ = ce.ref_detect(img, 5000, 0.01, 5.0)
    got, m = ref.ref_feature_detection_gftt(ce.strided(img, 131 + 29)[:, :131])     # rows 160 bytes apart, 0xEE between them
    assert m == n > 50 and np.array_equal(bits(got), bits(want))


def _oracle_chain_step(orc, state, l0, r0, l1, r1, P_l, P_r, K, mono=False):
    """the oracle's restated frame step (the chain tests/test_gpu_parity.py holds the product to)"""
    h, w = l0.shape
    if len(state["pts"]) < 2000:
        fast = orc.fast_detect(l0, 20, True)
        state["pts"] = np.vstack([state["pts"], fast])
        state["ages"] = np.concatenate([state["ages"], np.zeros(len(fast), np.int32)])
    bp, ba = orc.bucketing_features(h, w, state["pts"], state["ages"], h // 10, 1)
    cm = orc.circular_matching(l0, r0, l1, r1, bp, ages=ba)
    (pl0, pr0, pl1, pr1), _ = orc.check_valid_and_remove(cm["l0"], cm["r0"], cm["l1"], cm["r1"], cm["l0_ret"])
    state["pts"], state["ages"] = pl1, cm["ages"]
    xyz = orc.triangulate(P_l, P_r, pl0, pr0)
    rc, rv, tv, inl, _ = orc.solve_pnp_ransac(xyz, pl1, K, tvec=state["t"])
    state["t"] = tv
    Rm = orc.rodrigues(rv)
    if mono:
        focal, pp = float(P_l[0, 0]), (float(P_l[0, 2]), float(P_l[1, 2]))
        ok, E, mask, _ = orc.find_essential_mat(pl0, pl1, focal, pp)
        assert ok == 1
        _, Rm, _, _ = orc.recover_pose(E, pl0, pl1, focal, pp, mask)
    e = orc.rotation_matrix_to_euler(Rm)
    integrated = False
    if abs(e[1]) < 0.1 and abs(e[0]) < 0.1 and abs(e[2]) < 0.1:
        state["pose"], integrated = orc.integrate_odometry_stereo(state["pose"], Rm, tv)
    return dict(l0=pl0, r0=pr0, l1=pl1, r1=pr1, tvec=tv, R=Rm, integrated=integrated)


@pytest.mark.parametrize("mono", [False, True])
def test_frame_loop_restatement_equals_the_reference_sources(ref, small_world, mono):
    """matchingFeatures + triangulation + trackingFrame2Frame + euler gates + integrateOdometryStereo: the
    reference's own functions (oracle/_ref) and the oracle's restated chain, frame after frame on one sequence"""
    n = 5
    L, R, poses, _ = small_world.render_sequence(n)
    P_l, P_r = small_world.proj_matrices()
    K = small_world.K()
    loop = ref.RefFrameLoop(P_l[0, 0], P_l[0, 2], P_l[1, 2], P_r[0, 3], mono_rotation=mono)
    state = dict(pts=np.zeros((0, 2), np.float32), ages=np.zeros(0, np.int32), t=np.zeros(3), pose=np.eye(4))
    loop.process(L[0], R[0])
    for k in range(1, n):
        a = loop.process(L[k], R[k])
        b = _oracle_chain_step(ref, state, L[k - 1], R[k - 1], L[k], R[k], P_l, P_r, K, mono)
        for name in ("l0", "r0", "l1", "r1"):
            assert np.array_equal(bits(a[name]), bits(b[name])), (k, name)
        assert np.array_equal(bits(loop.points), bits(state["pts"])) and np.array_equal(loop.ages, state["ages"])
        assert np.array_equal(a["tvec"], b["tvec"]) and np.abs(a["R"] - b["R"]).max() == 0
        assert a["integrated"] == b["integrated"] and a["integrated"]
        assert np.abs(loop.frame_pose - state["pose"]).max() <= 1e-12   # different 4x4 inverse routines
    assert len(a["l1"]) > 20


def test_euler_and_integration_equal_the_reference_sources(ref):
    rng = np.random.default_rng(6)
    pose = np.eye(4)
    for _ in range(50):
        rv = rng.normal(0, 0.05, 3)
        Rm = ref.rodrigues(rv)
        t = rng.normal(0, 1, 3) * rng.choice([0.01, 1.0, 20.0])     # below / inside / above the scale gate
        assert np.array_equal(ref.rotation_matrix_to_euler(Rm), ref.ref_rotation_matrix_to_euler(Rm))
        p_ref = ref.ref_integrate_odometry_stereo(pose, Rm, t)
        p_orc, applied = ref.integrate_odometry_stereo(pose, Rm, t)
        assert applied == (0.05 < np.linalg.norm(t) < 10)
        assert np.abs(p_ref - p_orc).max() <= 1e-12 * max(1.0, np.abs(p_orc).max())
        pose = p_orc
