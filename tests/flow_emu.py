"""The one CPU-emulator harness of the two-image tracker (tests/host_check/flow_emu.cpp) as the tests use it: build, load, run,
parse.  Shared by test_flow_emulation.py, test_flow_win_emulation.py and test_flow_flags_emulation.py.

The library loaded into python is built WITHOUT sanitizer flags whatever the environment says.  The sanitizer tier is the same
harness as a STAND-ALONE program with its own main(): every pyramid level in an exactly sized heap block, built with
-fsanitize=address,undefined (runtimes linked statically) and run as a child.  Nothing instrumented is loaded into python."""
import ctypes as C

import numpy as np

import emu_build
from conftest import vp


def load():
    """libflow_emu.so, built when stale and loaded once per session"""
    lib = emu_build.shared("flow_emu")
    lib.fe_track.restype = C.c_int
    lib.fe_compact.restype = C.c_int
    return lib


def track(lib, c, flags=0, guess=None, want_err=True, n_frames=1, counts=None, frame=0, n=None, max_count=30):
    """the case's pair (prev, next, pts -- its first n --, win or 21, lk_max_level: the harness plans the levels) through the
    emulated kernel of its window and flags.  n_frames frames of one launch, or len(counts) frames that track the first counts[f]
    points; guess [n, 2] or one per frame.  Returns ((next, status, err or None), levels built): the outputs of frame `frame`,
    or with frame=None of every frame ([F, n, 2], [F, n], [F, n])"""
    prev, nxt = np.ascontiguousarray(c["prev"]), np.ascontiguousarray(c["next"])
    h, w = prev.shape
    pts = np.ascontiguousarray(c["pts"] if n is None else c["pts"][:n], np.float32).reshape(-1, 2)
    n, nf = len(pts), n_frames if counts is None else len(counts)
    io = np.zeros((nf, n, 2), np.float32)
    if guess is not None:
        io[:] = np.asarray(guess, np.float32).reshape(-1, n, 2)
    st = np.zeros((nf, n), np.uint8)
    err = np.zeros((nf, n), np.float32)
    cnt = None if counts is None else np.asarray(counts, np.int32)
    levels = lib.fe_track(vp(prev), vp(nxt), w, h, c["lk_max_level"], vp(pts), n, c.get("win", 21), flags, max_count, C.c_double(0.01),
                          C.c_float(1e-3), vp(io), vp(st), vp(err) if want_err else None, nf, None if cnt is None else vp(cnt))
    if frame is not None:
        io, st, err = io[frame], st[frame], err[frame]
    return (io, st, (err if want_err else None)), levels


def compact(lib, pts0, nxt, status, threads):
    n = len(status)
    st = status.copy()
    o0, o1 = np.zeros((max(n, 1), 2), np.float32), np.zeros((max(n, 1), 2), np.float32)
    idx = np.full(max(n, 1), -1, np.int32)
    k = lib.fe_compact(vp(np.ascontiguousarray(pts0, np.float32)), vp(np.ascontiguousarray(nxt, np.float32)), vp(st), n, vp(o0), vp(o1), vp(idx), threads)
    return o0[:k], o1[:k], st, idx[:k], k


def run_standalone(tmp_path, c, flags=0, guess=None, what=None):
    """the case (one frame) through the stand-alone ASan + UBSan program, run as a child: no report, exit status 0.  Returns
    (next, status, err) and the compaction of that result (n_out, the rewritten status, keep_idx)"""
    exe = emu_build.sanitized_program("flow_emu", "FLOW_EMU_MAIN")
    h, w = c["prev"].shape
    n = len(c["pts"])
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([w, h, c["lk_max_level"], n, c.get("max_count", 30), c.get("win", 21), flags], np.int32).tobytes())
        f.write(np.array([0.01], np.float64).tobytes() + np.array([1e-3], np.float32).tobytes())
        f.write(c["prev"].tobytes() + c["next"].tobytes() + c["pts"].tobytes())
        f.write(np.ascontiguousarray(c["pts"] if guess is None else guess, np.float32).tobytes())
    emu_build.run_clean(exe, [fin, fout], 600, what)
    raw = np.fromfile(fout, np.uint8)
    nxt = raw[:8 * n].view(np.float32).reshape(n, 2)
    err = raw[8 * n:12 * n].view(np.float32)
    st = raw[12 * n:13 * n]
    k = int(raw[13 * n:13 * n + 4].view(np.int32)[0])
    st2 = raw[13 * n + 4:14 * n + 4]
    idx = raw[14 * n + 4:14 * n + 4 + 4 * n].view(np.int32)[:k]
    return (nxt, st, err), (k, st2, idx)
