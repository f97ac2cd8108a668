"""cv::FAST under a mask (include/vo_fast_mask.h) on the CPU: the product's fast_mask_filter_kernel alone over synthetic lists at the
lengths where a chunked, wave-ranked compaction can go wrong, and the whole route of the frame loop -- seq_prepare_kernel, the FAST
kernels into a list of their own, corn_disc_frames_kernel, the filter, bucket_kernel's split form -- through the coroutine emulator
(tests/host_check/fast_mask_emu.cpp), in both orders the product launches them (inline, and FAST one step early as the lock-step
loop's look-ahead), against the composition of fast_mask_cases.py.  Identity throughout: the lists, the bucketed sets, the counts and
the planes against ref_disc_mask.  The same harness runs once more as a stand-alone program under ASan + UBSan."""
import numpy as np
import pytest

import corners_mask_cases as cm
import fast_mask_cases as fm

W, H, PAD = 37, 29, 3          # the synthetic planes: w x h with a pitch of w + 3; the padding holds 255


def lengths(chunk, cap):
    return sorted({0, 1, 63, 64, 65, chunk - 1, chunk, chunk + 1, 3 * chunk + 7, cap})


def synthetic_list(n, seed):
    """n list entries inside the plane, NOT sorted and with repeats: the kernel must keep the order it is given"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, W, n), rng.integers(0, H, n)], 1).astype(np.float32)


def plane_for(pts, keep):
    """a plane (H, W + PAD) that allows exactly the entries with keep[i] (entries that share a pixel share its fate: keep is made
    consistent first); the padding holds the opposite of what a wrong pitch would want to find"""
    keep = np.asarray(keep, bool).copy()
    plane = np.zeros((H, W + PAD), np.uint8)
    xy = pts.astype(int)
    allowed = {}
    for i, (x, y) in enumerate(xy):
        allowed.setdefault((x, y), keep[i])
    for i, (x, y) in enumerate(xy):
        keep[i] = allowed[(x, y)]
        plane[y, x] = 255 if keep[i] else 0
    plane[:, W:] = 255
    return plane, keep


def keep_patterns(n, chunk):
    pats = {"none": np.zeros(n, bool), "all": np.ones(n, bool), "alternating": np.arange(n) % 2 == 0}
    first, last, waves = np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, bool)
    if n:
        first[0] = last[-1] = True
    waves[63::64] = True
    waves[::64] = True           # entries 0, 63, 64, 127, 128, ...: both sides of every wave boundary
    pats.update(first=first, last=last, wave_boundaries=waves)
    return pats


def distinct_list(n, seed):
    """as synthetic_list, but every pixel at most once while the plane has room (so that "only the first" keeps exactly one)"""
    rng = np.random.default_rng(seed)
    cells = rng.permutation(W * H)
    idx = np.concatenate([cells] * (n // (W * H) + 1))[:n]
    return np.stack([idx % W, idx // W], 1).astype(np.float32)


@pytest.mark.parametrize("threads", [256, 1024])
def test_filter_kernel_at_the_lengths_where_it_can_go_wrong(threads):
    cap = 3 * threads + 40
    for n in lengths(threads, cap):
        for name, keep in keep_patterns(n, threads).items():
            pts = distinct_list(n, seed=n + threads)
            plane, keep = plane_for(pts, keep)
            if n <= W * H:
                assert keep.sum() == {"none": 0, "all": n, "first": min(n, 1), "last": min(n, 1)}.get(name, keep.sum()), (name, n)
            # frame 1 beside it: another count, and it does not detect -- its output stays untouched and its count is 0
            other = synthetic_list(min(cap, n + 5), seed=7)
            out, nout = fm.emu_filter([(pts, n), (other, len(other))], np.stack([plane, np.full_like(plane, 255)]), [1, 0], cap, threads)
            want = pts[keep]
            assert nout[0] == len(want), (name, n, nout[0], len(want))
            assert np.array_equal(out[0, :len(want)], want), (name, n)
            assert np.all(out[0, len(want):] == fm.SENTINEL), (name, n, "nothing behind the list is written")
            assert nout[1] == 0 and np.all(out[1] == fm.SENTINEL), (name, n)


@pytest.mark.parametrize("threads", [256, 1024])
def test_filter_kernel_two_detecting_frames_and_the_overflow_count(threads):
    cap = threads + 9
    a, b = synthetic_list(cap, 1), synthetic_list(threads - 1, 2)
    pa, ka = plane_for(a, np.arange(cap) % 3 == 0)
    pb, kb = plane_for(b, np.arange(len(b)) % 5 != 0)
    # frame 0 is told a count beyond the capacity: only cap entries exist, and the count that leaves is cap + 1
    out, nout = fm.emu_filter([(a, cap + 100), (b, len(b))], np.stack([pa, pb]), [1, 1], cap, threads)
    assert nout[0] == cap + 1 and np.array_equal(out[0, :ka.sum()], a[ka]) and np.all(out[0, ka.sum():] == fm.SENTINEL)
    assert nout[1] == kb.sum() and np.array_equal(out[1, :kb.sum()], b[kb]) and np.all(out[1, kb.sum():] == fm.SENTINEL)


IMAGES = {"crop32": lambda: fm.crop(fm.CROP_SMALL), "crop64": lambda: fm.crop(fm.CROP_BIG), "odd": lambda: fm.crop(fm.CROP_ODD), "L0": fm.L0}


def carried_for(img, name):
    h, w = img.shape
    if name == "L0":
        return fm.every_nth(img, 40)
    return fm.carried_set(w, h, 9, 2, seed=4)


def check_route(got, imgs, frames, radius, redetect_below=2000, fpb=1, bucket_size=0):
    for f, (image, pts, ages) in enumerate(frames):
        img = imgs[image]
        h, w = img.shape
        want_p, want_a, n_new = fm.expected_bucketed(img, pts, ages, radius, redetect_below, bucket_size, fpb)
        g = got[f]
        assert g["overflow"] == 0 and g["n_new"] == n_new and g["n"] == len(want_p), (f, g["n"], g["n_new"], n_new)
        assert np.array_equal(g["pts"], want_p) and np.array_equal(g["ages"], want_a), f
        assert g["detect"] == (1 if len(pts) < redetect_below else 0)
        if g["detect"]:
            assert np.array_equal(g["new"], fm.ref_topup_corners(img, pts, radius)), (f, "the masked list, in FAST's order")
            assert g["n_raw"] == len(fm.ref_fast(img))
            assert np.array_equal(g["plane"], cm.ref_disc_mask(w, h, pts, radius)), (f, "the plane against the header's disc mask")
        else:
            assert g["plane_touched"] == 0 and g["n_new"] == 0


@pytest.mark.parametrize("lookahead", [False, True], ids=["inline", "lookahead"])
@pytest.mark.parametrize("radius", [0, 5, 10])
@pytest.mark.parametrize("name", sorted(IMAGES))
def test_whole_route_against_the_composition(name, radius, lookahead):
    img = IMAGES[name]()
    pts, ages = carried_for(img, name)
    frames = [(0, pts, ages)]
    kw = dict(fpb=4 if name == "odd" else 1, filter_threads=256 if name == "crop64" else 1024)
    got = fm.emu_route([img], frames, radius=radius, lookahead=lookahead, **kw)
    check_route(got, [img], frames, radius, fpb=kw["fpb"])
    if name == "L0" and radius == 5:
        assert got[0]["n_raw"] - got[0]["n_new"] == 118


def case_frames():
    """three frames over two images: the middle one carries as many points as redetect_below and does not detect again; the last
    carries nothing (the unmasked call)"""
    imgs = [fm.crop(fm.CROP_BIG, 0), fm.crop(fm.CROP_BIG, 1)]
    full = fm.carried_set(64, 48, 30, 3, seed=6)
    return imgs, [(1,) + fm.carried_set(64, 48, 7, 1, seed=7), (0,) + full, (1,) + fm.EMPTY], dict(redetect_below=30)


@pytest.mark.parametrize("lookahead", [False, True], ids=["inline", "lookahead"])
def test_frames_that_do_not_detect_and_frames_that_carry_nothing(lookahead):
    imgs, frames, kw = case_frames()
    got = fm.emu_route(imgs, frames, radius=5, lookahead=lookahead, **kw)
    check_route(got, imgs, frames, 5, **kw)
    assert got[2]["n_new"] == got[2]["n_raw"] and not got[2]["plane_touched"]


def test_all_zero_mask_and_skipped_points():
    img = fm.crop(fm.CROP_SMALL)
    frames = [(0,) + fm.carried_set(32, 32, 40, 5)]
    got = fm.emu_route([img], frames, radius=10, bucket_threads=256)
    check_route(got, [img], frames, 10)
    assert got[0]["n_new"] == 0 and not got[0]["plane"].any() and got[0]["n_raw"] == 14
    big = fm.crop(fm.CROP_BIG)
    w, h = 64, 48
    pts = np.array([(np.nan, 5.0), (5.0, np.inf), (-np.inf, 3.0), (1e20, 4.0), (2.0 ** 30, 3.0), (20.5, 11.5), (-3.0, h / 2), (w + 2.0, h / 2), (w / 2, -4.0),
                    (40.2, 30.7)], np.float32)
    frames = [(0, pts, np.arange(len(pts) + 2, dtype=np.int32) % 13)]
    check_route(fm.emu_route([big], frames, radius=7), [big], frames, 7)


def test_overflow_of_the_unmasked_list():
    """the capacity is judged on the UNMASKED list: 72 corners against a list of 32, whatever the mask leaves, arrive at the bucketing as
    lcap + 1 and leave as bit 0 of the frame's overflow flag"""
    img = fm.crop(fm.CROP_BIG)
    pts, ages = fm.carried_set(64, 48, 40, 0, seed=2)
    assert len(fm.ref_topup_corners(img, pts, 10)) <= 32 < len(fm.ref_fast(img))
    for lookahead in (False, True):
        got = fm.emu_route([img], [(0, pts, ages)], radius=10, lcap=128, out_cap=512, lookahead=lookahead)
        assert got[0]["overflow"] == 0
        got = fm.emu_route([img], [(0, pts[:20], ages[:20])], radius=10, lcap=32, out_cap=512, lookahead=lookahead)
        assert got[0]["n_raw"] == 72 and got[0]["n_new"] == 33 and got[0]["overflow"] & 1


@pytest.mark.sanitize
def test_standalone_under_sanitizers(tmp_path):
    """the same harness as a stand-alone program built with -fsanitize=address,undefined, run as a child: the filter at both widths
    over the boundary lengths, and the route on the crops in both orders -- exit status 0, no report, the same bytes"""
    k = 0
    for threads in (256, 1024):
        cap = 3 * threads + 40
        for n in (0, 65, threads - 1, threads + 1, 3 * threads + 7, cap):
            pts = distinct_list(n, seed=n)
            plane, keep = plane_for(pts, keep_patterns(n, threads)["wave_boundaries" if n % 2 else "alternating"])
            d = tmp_path / ("f%d" % k)
            d.mkdir()
            k += 1
            out, nout = fm.emu_filter([(pts, n), (pts, n)], np.stack([plane, plane]), [1, 0], cap, threads, tmp_path=d)
            assert nout.tolist() == [keep.sum(), 0] and np.array_equal(out[0, :keep.sum()], pts[keep]) and np.all(out[1] == fm.SENTINEL)
    for name in ("crop32", "odd"):
        for lookahead in (False, True):
            img = IMAGES[name]()
            frames = [(0,) + carried_for(img, name)]
            d = tmp_path / ("r_%s_%d" % (name, lookahead))
            d.mkdir()
            check_route(fm.emu_route([img], frames, radius=5, lookahead=lookahead, tmp_path=d), [img], frames, 5)
    imgs, frames, kw = case_frames()
    d = tmp_path / "frames"
    d.mkdir()
    check_route(fm.emu_route(imgs, frames, radius=5, lookahead=True, tmp_path=d, **kw), imgs, frames, 5, **kw)
