"""rectify_kernel (visual_odom_amd/csrc/rectify.hip) executed on the CPU through the coroutine SIMT emulator
(tests/host_check/hip_emu.h + rectify_emu.cpp), behind the product's own map packing (vo_rectify.h), and compared BIT FOR BIT
with the numpy restatement of the formula of include/vo_hip.h (tests/rectify_cases.py: remap_ref).

Shapes: w in {32, 33, 39, 64, 519} (multiples of 4 and not, one and three 256-pixel runs) x h in {32, 37}; destination pitch
greater than w with the bytes outside the w columns checked (guard pattern); fewer and more waves than rows.  Maps: identity,
all 32 x 32 weight pairs, half-even ties, a barrel map whose corners leave the image, and edge entries (-1, -0.5, -1/32, w - 1,
w - 1 + 1/32, w, +-1e6, NaN, +-inf in x and in y).  Both sides in every launch, with different maps.

The sanitizer tier is a STAND-ALONE program: the same harness with a main() of its own, every raw plane and the packed maps in
exactly sized heap blocks, built with -fsanitize=address,undefined (the runtimes linked statically: the program carries them and
starts in whatever environment the suite runs in, which it inherits unchanged apart from the sanitizers' own option variables)
and run as a child over the barrel and edge cases.  Nothing instrumented is loaded into python.  Unit test of device code, not a product path."""
import ctypes as C

import numpy as np
import pytest

import emu_build
from conftest import BUILD_DIR, SAN_FLAGS, vp
from rectify_cases import HEIGHTS, MAP_KINDS, WIDTHS, make_image, make_maps, remap_ref

GUARD = 0xA5


@pytest.fixture(scope="module")
def rfe():
    lib = emu_build.shared("rectify_emu", SAN_FLAGS, BUILD_DIR)
    lib.rfe_pack.restype = C.c_int
    lib.rfe_rectify.restype = C.c_int
    return lib


def pack(rfe, maps, w, h):
    packed = np.zeros((2, h, w), np.uint32)
    for side, (mx, my) in enumerate(maps):
        assert rfe.rfe_pack(vp(mx), vp(my), w, w, h, vp(packed[side])) == 0
    return packed


def case(kind, w, h):
    rng = np.random.default_rng(7919 * w + 31 * h + MAP_KINDS.index(kind))
    maps = [make_maps(kind, w, h, side) for side in (0, 1)]
    sides = [0, 1, 1, 0]   # (two pairs' worth, the second one swapped: the table's side decides, not the position)
    imgs = [make_image(rng, w, h) for _ in sides]
    want = np.stack([remap_ref(img, *maps[s]) for img, s in zip(imgs, sides)])
    return maps, sides, imgs, want


@pytest.mark.parametrize("kind", MAP_KINDS)
@pytest.mark.parametrize("h", HEIGHTS)
@pytest.mark.parametrize("w", WIDTHS)
def test_rectify_kernel(rfe, w, h, kind):
    maps, sides, imgs, want = case(kind, w, h)
    packed = pack(rfe, maps, w, h)
    pitch = (32 + w + 24 + 15) // 16 * 16
    if kind == "identity":
        assert np.array_equal(want[0], imgs[0])
    for n_waves in (3, len(imgs) * h * ((w + 255) // 256) + 11):   # fewer and more waves than rows
        dst = np.full((len(imgs), h, pitch), GUARD, np.uint8)
        src = (C.c_void_p * len(imgs))(*[i.ctypes.data for i in imgs])
        rc = rfe.rfe_rectify(src, vp(np.array(sides, np.int32)), len(imgs), w, h, vp(packed), pitch, vp(dst), n_waves)
        assert rc == 0
        assert np.array_equal(dst[:, :, :w], want)
        assert np.all(dst[:, :, w:] == GUARD), "a destination byte outside the w columns of a row changed"


def test_all_weight_pairs_and_ties_are_what_they_claim():
    """the cases' own premises: every (a, b) pair occurs; the tie entries land on .5 of the 1/32 grid and round to even"""
    mx, my = make_maps("all_ab", 64, 37)
    a = np.rint(mx * 32).astype(int)[:32, :32] & 31
    b = np.rint(my * 32).astype(int)[:32, :32] & 31
    assert len(set(zip(a.ravel().tolist(), b.ravel().tolist()))) == 1024
    mx, _ = make_maps("ties", 32, 32)
    frac = (mx.astype(np.float64) * 32) % 1
    assert np.all(frac == 0.5)
    assert set((np.rint(mx * np.float32(32)).astype(int) & 31).ravel().tolist()) == {0, 2}


def test_pack_refuses_a_far_displacement_that_is_inside(rfe):
    """more than 1023 pixels from its own pixel and not wholly outside: cannot be packed (vo_set_params: VO_ERR_ARG); the
    same entry wholly outside is the reserved pattern"""
    w, h = 1100, 32
    mx, my = make_maps("identity", w, h)
    out = np.zeros((h, w), np.uint32)
    mx[5, 1090] = 10.0
    assert rfe.rfe_pack(vp(mx), vp(my), w, w, h, vp(out)) == -1
    mx[5, 1090] = -30.0
    assert rfe.rfe_pack(vp(mx), vp(my), w, w, h, vp(out)) == 0 and out[5, 1090] == 0x80008000
    mx[5, 1090] = 1090 - 1023.0
    assert rfe.rfe_pack(vp(mx), vp(my), w, w, h, vp(out)) == 0 and out[5, 1090] == ((-1023 * 32) & 0xffff)


@pytest.mark.sanitize
@pytest.mark.parametrize("kind", ["barrel", "edges"])
def test_rectify_kernel_standalone_under_sanitizers(tmp_path, kind):
    """ASan + UBSan over the kernel source and the packing in a program of its own: exactly sized raw planes and maps, no report"""
    exe = emu_build.sanitized_program("rectify_emu", "RECTIFY_EMU_MAIN")
    for w, h in ((33, 37), (519, 32), (64, 32)):
        maps, sides, imgs, want = case(kind, w, h)
        pitch, n_waves = (32 + w + 24 + 15) // 16 * 16, 7
        fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(fin, "wb") as f:
            f.write(np.array([len(imgs), w, h, pitch, n_waves, GUARD], np.int32).tobytes())
            f.write(np.array(sides, np.int32).tobytes())
            for mx, my in maps:
                f.write(mx.tobytes() + my.tobytes())
            f.write(np.stack(imgs).tobytes())
        emu_build.run_clean(exe, [fin, fout], 300)
        dst = np.fromfile(fout, np.uint8).reshape(len(imgs), h, pitch)
        assert np.array_equal(dst[:, :, :w], want)
        assert np.all(dst[:, :, w:] == GUARD)
