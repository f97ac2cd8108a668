"""vo_lkmath.h's vertical-pair samplers on the host: lift8_cols + blend7_cols equals bilinear7_u8, and bilinear7_deriv_cols
equals bilinear7_deriv, bit for bit, and both equal the plain int64 DESCALE formula -- over a grid of weight pairs that holds
iw11 = -1 (the three rounded weights adding up to 2^14 + 1) and pixel bytes all 0 / all 255 / alternating / random, Scharr samples
at +-16320 / random (tests/host_check/lk_cols_cases.h has the list).  A small g++ program: the `#else` text of the wrappers."""
import lk_cols


def test_vertical_pair_samplers_equal_the_horizontal_ones(tmp_path):
    exe = lk_cols.build_host(str(tmp_path))
    n, n_neg = lk_cols.run(exe, str(tmp_path / "host.out"))
    print("lk_cols_host: %d cases, %d with iw11 < 0" % (n, n_neg))
    assert n >= 30000 and n_neg >= 100 and n % 8 == 0
