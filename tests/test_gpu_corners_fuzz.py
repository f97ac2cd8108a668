"""The seeded fuzz of the Shi-Tomasi detector on the device (the generator, its checks and its floors: corners_fuzz_cases.py).
tools/gpu_round.sh hunt re-runs it longer and with other seeds (VO_FUZZ_EXAMPLES, VO_FUZZ_SEED)."""
import os

import pytest

import corners_fuzz_cases as cf

pytestmark = pytest.mark.gpu


def test_corners_fuzz(volib):
    """300 random cases through vocorn_min_eigen_map (every fifth), vocorn_detect (every one), vocmask_detect under a random mask
    (every third) and vocmask_replenish around random kept points (every seventh): a region of interest of seven 640 x 256 sources
    as a view with stride 640, widths on both sides of the map kernel's seams, distances from 0 to 256 around the shortcut and the
    half-to-even cell sizes, lists up to the capacity of 16 384 and beyond it (refused, nothing written: counted under "over",
    never skipped) -- map, corners and their order BIT-EXACT against tests/host_check/corners_ref.c and, under a mask,
    corners_mask_cases.ref_detect.  Measured on an MI355X: 3.0 .. 4.5 s for the 300 cases, references included (the default seed
    with every test module collected: 284 compared, 16 refused, 115 lists beyond 2 048 candidates, 91 under a mask, 24 replenished,
    174 558 corners)."""
    ctx = volib.Context(0, cf.SRC_W, cf.SRC_H, 256, 1)
    try:
        seen = cf.run(cf.DeviceBackend(ctx, volib, cf.SRC_W, cf.SRC_H), explore=os.environ.get("VO_FUZZ_SEED"))
    finally:
        ctx.close()
    print("corners fuzz:", seen)
    cf.check_floors(seen)
