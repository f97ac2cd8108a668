"""The vectors of tests/host_check/lk_cols_cases.h through lift8_cols + blend7_cols and bilinear7_deriv_cols on gfx950
(tests/host_check/lk_cols_check.hip: one small program, built with the product's flags, started ONCE).  The program compares
the device's records with its own host pass of the same composites, of bilinear7_u8 / bilinear7_deriv and of the plain formula;
here the records it wrote are compared, byte for byte, with what the g++ build (lk_cols_host.cpp) wrote."""
import numpy as np
import pytest

import lk_cols

pytestmark = pytest.mark.gpu


def test_vertical_pair_samplers_on_the_device(tmp_path):
    d = str(tmp_path)
    host, dev = lk_cols.build_host(d), lk_cols.build_device(d)
    n_host = lk_cols.run(host, str(tmp_path / "host.out"))
    n_dev = lk_cols.run(dev, str(tmp_path / "dev.out"))       # a non-zero exit, a signal or the time limit fails here: no second run
    assert n_dev == n_host and n_dev[1] >= 100
    want = np.fromfile(str(tmp_path / "host.out"), np.uint32).reshape(-1, 12)
    got = np.fromfile(str(tmp_path / "dev.out"), np.uint32).reshape(-1, 12)
    bad = np.flatnonzero((got != want).any(1))
    assert len(bad) == 0, ("device != g++ build", len(bad), int(bad[0]), got[bad[0]], want[bad[0]])
