"""tests/pyramid_planes.py on the CPU: the premises of its expectation, and pyr_pass_kernel on the emulator in both regimes of the
product (wide border items in XCD-aware order; thin ones in dispatch order) against it at every shape the device test uses, every
byte of every level's planes.  tests/test_gpu_pyramid_planes.py holds the MI355X to the same expectation: a failure there that
does not show here is the device's or the host layer's, not the kernel source's."""
import numpy as np
import pytest

import pyramid_planes as pp


@pytest.mark.parametrize("shape", pp.SHAPES, ids=pp.ids)
def test_expectation_premises(orc, shape):
    """the border is neither a replicated edge nor (at the narrow and low levels) a single reflection, der has both signs, the
    checkerboard reaches +-16320; two images of a batch differ in every plane"""
    for k in (0, 1):
        pp.premises(shape, pp.expected(orc, shape, k))
    pp.premises(shape, pp.expected(orc, shape, 3), is_checker=True)
    for (p0, d0), (p1, d1) in zip(pp.expected(orc, shape, 0), pp.expected(orc, shape, 1)):
        assert (p0 != p1).mean() > 0.5 and (d0 != d1).any()


def test_shapes_reach_what_they_are_chosen_for():
    lv = {s: [pp.level_shape(s, l) for l in range(pp.depth(*s) + 1)] for s in pp.SHAPES}
    assert lv[(32, 32)] == [(32, 32)]
    assert lv[(47, 45)][-1] == (24, 23) and lv[(45, 47)][-1] == (23, 24)
    assert len(lv[(131, 97)]) == 3 and lv[(169, 169)] == [(169, 169), (85, 85), (43, 43), (22, 22)]
    assert (301 + 3) // 4 > 64 and lv[(301, 45)][-1][1] == 23
    assert [s[0] % 16 for s in pp.SHAPES[-4:]] == [9, 9, 15, 8]
    assert {w % 4 for levels in lv.values() for w, _ in levels} == {0, 1, 2, 3}      # (w mod 4 = 2: 66 and 22, levels of the two big shapes)


@pytest.mark.parametrize("regime", sorted(pp.REGIMES))
@pytest.mark.parametrize("shape", pp.SHAPES, ids=pp.ids)
def test_emulated_planes(orc, shape, regime):
    lib = pp.emu_lib()
    for k in (0, 3):
        pp.assert_planes(pp.emu_planes(lib, pp.image(shape, k), 3, pp.REGIMES[regime]), pp.expected(orc, shape, k), (shape, regime, k))
    two = pp.emu_planes(lib, pp.image(shape, 1), 1, pp.REGIMES[regime])      # lk_max_level = 1: the reconfigure test's depth
    pp.assert_planes(two, pp.expected(orc, shape, 1, 1), (shape, regime, "two levels"))
    assert len(two) == min(2, pp.depth(*shape) + 1)
