"""The Shi-Tomasi detector on the device where corn_select_kernel and corn_map_kernel change behaviour: the table of corners_scale.py
through vocorn_min_eigen_map, vocorn_detect and vocmask_detect, held BIT FOR BIT, order included, to the reference, after each case's
premise has been asserted from the reference alone.  The concurrent parts of corn_select_kernel -- the sort's barriers over global
keys across 16 waves, the unsynchronised stamps of st[], the rotating LDS flag, loops of several trips -- run concurrently only
here: the emulator tier (test_corners_scale_emulation.py) runs the same table one thread after the other.

A context of 512 x 132 pixels and 256 points has the default corner-list capacity of 16 384: the full list fills it exactly, one
candidate more is refused with nothing written, and the next call is not affected."""
import ctypes as C
import os

import numpy as np
import pytest

import corners_emu as ce
import corners_fuzz_cases as cf
import corners_mask_cases as cm
import corners_scale as cs

pytestmark = pytest.mark.gpu

MAX_W, MAX_H, MAX_PTS = 512, 132, 256


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def ctx(volib):
    c = volib.Context(0, MAX_W, MAX_H, MAX_PTS, 4)
    yield c
    c.close()


@pytest.fixture(scope="module")
def dev(ctx, volib):
    return cf.DeviceBackend(ctx, volib, MAX_W, MAX_H)


def padded(a, extra=5):
    """the array as a view of a wider one: a byte stride that is not the width"""
    h, w = a.shape
    buf = np.full((h, w + extra), 0xEE, np.uint8)
    buf[:, :w] = a
    return buf[:, :w]


def test_the_context_has_the_default_capacity(dev):
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vo_hip.h")).read()
    assert "max(4 * max_pts, 16384, max_w * max_h / 16)" in text
    assert dev.capacity == max(4 * MAX_PTS, 16384, MAX_W * MAX_H // 16) == cs.CAPACITY


@pytest.mark.parametrize("group", list(cs.GROUPS))
def test_scale_cases_bit_for_bit(ctx, dev, group):
    mapped = set()
    for c in cs.GROUPS[group]:
        want, n, ncand = cs.premise(c)
        h, w = c.img.shape
        img = padded(c.img)
        everything = padded(np.full((h, w), 255, np.uint8), 9)   # vocmask_detect under a mask that allows every pixel: the masked kernels
        if id(c.img) not in mapped:                              # the quality map, once per image
            mapped.add(id(c.img))
            assert np.array_equal(bits(ctx.corner_min_eigen_val(img)), bits(cs.ref_map(c))), c.name
        for mask in (None, everything):
            got = dev.detect(img, mask, c.max_corners, c.quality, c.min_distance)
            if c.over:
                assert got is None, (c.name, "accepted beyond the capacity")
                continue
            assert got is not None and got[1] == n and np.array_equal(got[0], want), (c.name, mask is not None, "corner list or its order differs")


@pytest.mark.parametrize("name", [m[0] for m in cs.MASK_CASES])
def test_plateau_under_a_mask(dev, name):
    _, img, mask, mc, q, md = next(m for m in cs.MASK_CASES if m[0] == name)
    want, n, _ = cs.mask_ref(name)
    got = dev.detect(padded(img), mask, mc, q, md)
    assert got is not None and got[1] == n and np.array_equal(got[0], want)


def test_the_exact_boundary(ctx, dev, volib):
    """16 384 candidates come back complete; 16 385 are refused, n_out and the buffer untouched; then 16 384 again"""
    full, over = cs.GROUPS["full-list"][0], cs.GROUPS["one-over"][0]
    want, n, ncand = cs.premise(full)
    assert n == ncand == cs.CAPACITY and cs.premise(over)[2] == cs.CAPACITY + 1
    got = dev.detect(padded(full.img), None, 0, full.quality, 0.0)
    assert got is not None and got[1] == cs.CAPACITY and np.array_equal(got[0], want)
    pts = np.full((cs.CAPACITY + 8, 2), -5, np.float32)
    cnt = C.c_int(-77)
    prm = volib.VoCornParams(0, over.quality, 0.0)
    img = padded(over.img)
    rc = ctx.lib.vocorn_detect(ctx.h, img.ctypes.data, 256, 132, img.strides[0], C.byref(prm), pts.ctypes.data, len(pts), C.byref(cnt))
    assert rc == volib.VO_ERR_OVERFLOW and cnt.value == -77 and (pts == -5).all() and b"capacity" in ctx.lib.vo_last_error(ctx.h)
    again = dev.detect(padded(full.img), None, 0, full.quality, 0.0)
    assert again is not None and again[1] == cs.CAPACITY and np.array_equal(again[0], want)
    assert np.array_equal(ctx.good_features_to_track(padded(full.img), 0, full.quality, 0.0), want)   # (the binding fetches twice: 8 192, then all)


def test_batch_of_four_long_lists_and_one_under_a_mask(ctx, volib):
    """four slots at 256 x 132: the full list, one candidate too many, noise, one short of full.  The key lists are kcap apart, the
    stamps and the corners lcap: with long lists a wrong stride lands in the neighbour's"""
    w, h = 256, 132
    full, over, short = cs.GROUPS["full-list"][0], cs.GROUPS["one-over"][0], cs.GROUPS["one-short"][0]
    imgs = [full.img, over.img, ce.noise(w, h, 31), short.img]
    mask = cm.checker(w, h)
    ctx.batch_configure(4, w, h, 1)
    for i, img in enumerate(imgs):
        ctx.batch_upload_image(i, padded(img))

    def refused(i):
        out = np.full((8, 2), -5, np.float32)
        n = C.c_int(-77)
        return (ctx.lib.vocorn_batch_get(ctx.h, i, out.ctypes.data, 8, C.byref(n)) == volib.VO_ERR_OVERFLOW and n.value == -77 and (out == -5).all())

    for md in (1.2, 5.0):
        wants = {i: ce.ref_detect(imgs[i], 0, 0.01, md) for i in (0, 2, 3)}
        assert wants[0][2] == 16384 and wants[3][2] == 16383 and ce.ref_detect(imgs[1], 0, 0.01, md)[2] == 16385 and 1024 < wants[2][2] < 16384
        ctx.corners_batch_run(0, 4, 0, 0.01, md)
        assert refused(1)
        for i in (3, 0, 2):
            got, m = ctx.corners_batch_get(i, cap=cs.CAPACITY)
            assert m == wants[i][1] and np.array_equal(got, wants[i][0]), (md, i)
        # slot 3 under a mask, the others as they were
        mwant, mn, mcand = cm.ref_detect(imgs[3], mask, 0, 0.01, md)
        assert 2048 < mcand < 16383 and 0 < mn < wants[3][1]
        ctx.corners_batch_set_mask(3, padded(mask, 3))
        ctx.corners_batch_run(0, 4, 0, 0.01, md, masked=True)
        got, m = ctx.corners_batch_get(3, cap=cs.CAPACITY)
        assert m == mn and np.array_equal(got, mwant), md
        assert refused(1)
        for i in (0, 2):
            got, m = ctx.corners_batch_get(i, cap=cs.CAPACITY)
            assert m == wants[i][1] and np.array_equal(got, wants[i][0]), (md, i)
        ctx.corners_batch_set_mask(3, None)
