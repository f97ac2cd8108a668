"""The bilinear weights and the blend with the caller's word on the sign of iw11, on the host (tests/host_check/lk_weights_host.cpp, a
g++ program with its own main over the text of vo_lkmath.h that the CPU emulator runs):
(a) lk_weights_packed -- (a * b1, b * a1) as a pair into the packed scale-and-round, a1 * b1 beside it -- equals the statement it
    replaced and OpenCV's plain one bit for bit, by column and by row, on 155 122 fraction pairs: two dense grids (256 x 256 and
    251 x 251), every pair of the 64 smallest and the 64 largest floats of [0, 1), and 101 x 101 pairs around 3.0e-5 .. 3.25e-5,
    where iw11 = -1;
(b) blend7_cols told the sign equals blend7_cols that tests it per lane and bilinear7_u8 on random cells.
At least 100 pairs and 100 blends take iw11 = -1 (the program's own assertion, repeated here on its numbers).
The second test is the same program under AddressSanitizer and UBSan -- a stand-alone child, nothing instrumented is loaded into
python."""
import subprocess

import lk_branches


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, "%s exited with %d:\n%s\n%s" % (exe, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    word = r.stdout.split()
    assert word[0] == "OK", r.stdout
    pairs, neg, blends, blend_neg = [int(x) for x in word[1:]]
    print("lk_weights_host: %d fraction pairs, %d with iw11 = -1; %d blends, %d with iw11 = -1" % (pairs, neg, blends, blend_neg))
    assert pairs == lk_branches.HOST_PAIRS
    assert neg >= 100 and blend_neg >= 100 and blends >= 128 * 128 + 101 * 101


def test_weights_and_blend_on_the_host(tmp_path):
    _run(lk_branches.build_host(str(tmp_path)))


def test_weights_and_blend_under_sanitizers(tmp_path):
    _run(lk_branches.build_host(str(tmp_path), sanitize=True))
