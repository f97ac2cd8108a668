"""The Shi-Tomasi kernels (visual_odom_amd/csrc/corners.hip) through the coroutine emulator at the sizes where corn_select_kernel and
corn_map_kernel change behaviour -- the table of corners_scale.py: a list that fills the default capacity of 16 384 exactly, one
short of it and one over, a plateau of 3 528 candidates (no power of two) with more than a hundred suppression rounds, the seam
widths of the map kernel, distances around the `lim <= 1` shortcut and the half-to-even cell sizes, max_corners inside a long list,
the plateau under a mask -- held BIT FOR BIT to the reference, after each case's premise has been asserted from the reference alone.
Then forty cases of the seeded fuzz of test_gpu_corners_fuzz.py, and that fuzz's floors from the reference alone.

The emulator runs the threads of a block one after the other: it checks the kernels' logic at these sizes (every strided loop makes
several trips, the sort pads, the scan's chunks are longer than 1), and tells a logic error apart from a device-only one when
test_gpu_corners_scale.py fails.  CPU only."""
import numpy as np
import pytest

import corners_emu as ce
import corners_fuzz_cases as cf
import corners_mask_cases as cm
import corners_scale as cs


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("group", list(cs.GROUPS))
def test_scale_cases_bit_for_bit(group):
    mapped = set()
    for c in cs.GROUPS[group]:
        want, n, ncand = cs.premise(c)
        h, w = c.img.shape
        pts, got_n, got_cand, rounds = ce.emu_detect([c.img], c.max_corners, c.quality, c.min_distance, cap=cs.CAPACITY, lcap=cs.CAPACITY, stride=w + 3)[0]
        assert got_cand == ncand, c.name
        if id(c.img) not in mapped:                            # the quality map, once per image
            mapped.add(id(c.img))
            assert np.array_equal(bits(ce.emu_map(c.img, stride=w + 5)), bits(cs.ref_map(c))), c.name
        if c.over:
            assert got_n == -1 and len(pts) == 0, c.name       # the overflow mark, no corners
            continue
        assert got_n == n and np.array_equal(pts, want), (c.name, "corner list or its order differs")
        if c.deep:
            assert rounds >= 100, (c.name, rounds)             # so the case cannot silently stop being deep


def test_capacity_is_a_property_of_the_list_not_of_the_image():
    """the full list in a list of exactly its length and of one less: 16 384 corners, and the overflow mark"""
    c = cs.GROUPS["full-list"][0]
    want, n, ncand = cs.premise(c)
    assert ce.emu_detect([c.img], 0, c.quality, 0.0, cap=1, lcap=ncand - 1, stride=259)[0][1] == -1
    short = cs.GROUPS["one-short"][0]
    pts, got_n, _, _ = ce.emu_detect([short.img], 0, short.quality, 0.0, cap=cs.CAPACITY, lcap=16383, stride=259)[0]   # the sort still runs over 16 384 keys
    assert got_n == 16383 and np.array_equal(pts, cs.premise(short)[0])


@pytest.mark.parametrize("name", [m[0] for m in cs.MASK_CASES])
def test_plateau_under_a_mask(name):
    _, img, mask, mc, q, md = next(m for m in cs.MASK_CASES if m[0] == name)
    want, n, ncand = cs.mask_ref(name)
    pts, got_n, got_cand = cm.emu_detect([img], [mask], mc, q, md, cap=cs.CAPACITY, lcap=cs.CAPACITY, stride=img.shape[1] + 3, mask_stride=img.shape[1] + 9)[0]
    assert (got_n, got_cand) == (n, ncand) and np.array_equal(pts, want)


def test_standalone_under_asan_and_ubsan_with_a_list_that_is_no_power_of_two(tmp_path):
    """the plateau of 3 528 candidates at distance 1.2 through the stand-alone ASan + UBSan program (a child with its own main();
    nothing instrumented is loaded into python) with lcap = its candidate count: keys, cell keys, stamps and corners in heap blocks
    of exactly that length (the two key lists: the power of two above it), 118 rounds, four trips of every strided loop"""
    c = cs.GROUPS["plateau"][0]
    want, n, ncand = cs.premise(c)
    eig, res = ce.run_standalone(tmp_path, [c.img], 0, c.quality, c.min_distance, cap=ncand, lcap=ncand, stride=c.img.shape[1] + 3)
    assert np.array_equal(bits(eig), bits(ce.ref_map(c.img)))
    pts, got_n, got_cand, rounds = res[0]
    assert (got_n, got_cand) == (n, ncand) and rounds >= 100 and np.array_equal(pts, want)


def test_fuzz_floors_hold_for_the_reference_alone():
    """the default run of test_gpu_corners_fuzz.py with nothing under test: the generator's value lists reach every floor"""
    seen = cf.run(None, n_examples=300)
    print("corners fuzz (reference alone):", seen)
    cf.check_floors(seen)


def test_forty_fuzz_cases_through_the_emulator():
    seen = cf.run(cf.EmuBackend(), n_examples=40)
    print("corners fuzz (emulator):", seen)
    assert seen["examples"] >= 40 and seen["cases"] >= 30 and seen["masked"] + seen["replenished"] > 0, seen
