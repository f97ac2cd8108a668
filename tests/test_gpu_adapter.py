"""The shipped adapter's entry points that no other test runs -- featureTracking_hip, featureDetectionGoodFeaturesToTrack_hip,
goodFeaturesToTrack_hip -- and its process-global state (the kept pair, the context that is re-created when it has to grow), on the
MI355X against the reference's own functions on the CPU: tests/adapter_cases.py, run ONCE in a fresh child process (the adapter's
context belongs to the process and other tests use it; a death of the child fails these tests and nothing else).  Every comparison
is identity; a check named "premise ..." is about the expected side alone and has to hold as well."""
import json
import os
import subprocess
import sys
import zlib

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


NEEDS = ("adapter_last_error", "adapter_feature_tracking", "adapter_gftt_default", "adapter_gftt", "adapter_circular_matching",
         "ref_delete_unmatch_features", "ref_feature_tracking", "ref_feature_detection_gftt")


@pytest.fixture(scope="module")
def run(orc):
    so = orc.build_ref_dropin()   # (re)built from this tree's sources where the reference tree is; elsewhere what travelled here
    if orc.ref_lib() is None or so is None:
        pytest.skip("oracle/_ref/libvo_ref_dropin.so is built only where the reference tree exists (make -C oracle/ref_dropin)")
    import ctypes
    libs = (ctypes.CDLL(so), orc.ref_lib())
    missing = [s for s in NEEDS if not any(hasattr(lib, s) for lib in libs)]
    if missing:
        # the libraries of oracle/_ref cannot be built here (no reference tree) and the ones that travelled here were built from
        # another commit's glue sources: they say nothing about this tree
        assert not orc.can_build_ref(), "oracle/_ref was built from this tree just now and lacks %s" % missing
        pytest.skip("oracle/_ref was built from another commit's glue sources (no %s) and cannot be rebuilt here" % ", ".join(missing))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "adapter_cases.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode in (0, 1) and r.stdout.strip(), "adapter_cases died (rc %d): %s" % (r.returncode, r.stderr[-2000:])
    return r


def group(run, prefix, count):
    """the checks of a group, all of them true: the child ended by itself, and none of the group's checks is missing"""
    assert run.returncode in (0, 1), "adapter_cases died (rc %d): %s" % (run.returncode, run.stderr[-2000:])
    rep = json.loads(run.stdout.strip().splitlines()[-1])
    got = {k: v for k, v in rep["checks"].items() if k.startswith(prefix) or k.startswith("premise " + prefix)}
    bad = {k: rep["details"].get(k) for k, v in got.items() if not v}
    assert not bad, bad
    assert len(got) == count, sorted(got)
    return got


def test_the_child_saw_the_session_frames(run, small_seq):
    assert run.returncode in (0, 1), "adapter_cases died (rc %d): %s" % (run.returncode, run.stderr[-2000:])
    rep = json.loads(run.stdout.strip().splitlines()[-1])
    import numpy as np
    arrays = [np.ascontiguousarray(a, np.uint8) for a in small_seq["L"] + small_seq["R"]] + [np.ascontiguousarray(p, np.float32) for p in small_seq["pts"]]
    assert rep["inputs"] == zlib.crc32(b"".join(a.tobytes() for a in arrays))


def test_context_growth_keeps_every_call_right(run):
    """96 x 64, 480 x 160 (re-created), 96 x 64, more than 16 384 points (re-created), then circularMatching_hip on buffers whose
    pair an earlier context kept: every call equals the reference, none counts as kept"""
    got = group(run, "growth", 9)
    assert "growth 4: featureTracking_hip with more than 16 384 points" in got and "growth 5: not counted as kept" in got


def test_feature_tracking_hip_equals_the_reference_function(run):
    """points1, points2, status and their lengths == featureTracking (feature.cpp:64-74): L0-L1, L0-R0, the 96 x 64 lattice, n = 0,
    views with step != cols"""
    got = group(run, "tracking", 8)
    for name in ("L0-L1", "L0-R0", "lattice", "n = 0", "L0-R0 as views with step != cols"):
        assert "tracking " + name in got


def test_feature_detection_gftt_hip_equals_the_reference_function(run):
    """== featureDetectionGoodFeaturesToTrack (feature.cpp:49-62): noise, blobs, L0, a padded step, the 5000 limit binding, a
    vector that is not empty on entry"""
    got = group(run, "detection", 11)
    assert "detection limit binds" in got and "detection with a padded step" in got and "detection into a vector that holds points" in got


def test_good_features_to_track_hip_equals_the_masked_reference(run):
    """== corners_mask_cases.ref_detect: no mask, a mask, a mask view, maxCorners 17, maxCorners 0 / -1 beyond the adapter's first
    buffer (the second vocmask_detect call), candidates beyond the capacity, and the call after it"""
    got = group(run, "corners", 14)
    for name in ("maxCorners 0: all of them come back", "maxCorners -1 under a mask: all of them come back", "under a mask with step != cols",
                 "beyond the capacity: refused, the text names the capacity", "after the refusal"):
        assert "corners " + name in got


def test_good_features_to_track_hip_refuses_what_it_documents(run):
    got = group(run, "refusal", 4)
    assert sorted(got) == ["refusal: a mask of another height", "refusal: a mask of another size", "refusal: a mask that is not CV_8UC1",
                           "refusal: an image that is not 8-bit"]


def test_kept_pair_across_the_other_entry_points(run):
    """keep_pair on: A, featureDetectionGoodFeaturesToTrack_hip, B on A's t1 buffers -> one kept call, B right; with
    featureTracking_hip between -> none, B right"""
    got = group(run, "state", 9)
    assert "state, featureDetectionGoodFeaturesToTrack_hip between: kept calls grow by 1" in got
    assert "state, featureTracking_hip between: kept calls grow by 0" in got
