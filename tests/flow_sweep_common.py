"""What the argument sweeps of the two-image tracker (flow_sweep.py, flow_win_sweep.py, flow_flags_sweep.py) share: the context, the
sentinel-filled buffers, `expect` -- one counted call that must come back with the documented code and, refused, leave vo_last_error
filled --, `untouched` and the JSON report {"checked": n, "covered": [...], "failures": [...]}.  Needs a GPU (vo_create)."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from visual_odom_amd import _lib  # noqa: E402

OK, ARG, STATE = 0, -1, -3
W, H, CAP, FRAMES = 320, 96, 256, 2
SENT = 77.25


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


class Sweep:
    def __init__(self, no_message=()):
        """no_message: calls whose refusal leaves vo_last_error as it was"""
        self.lib = _lib.load()
        self.fails, self.covered, self.checked, self.no_message = [], set(), 0, no_message
        self.ctx = _lib.Context(0, W, H, CAP, FRAMES)
        self.h = self.ctx.h
        rng = np.random.default_rng(3)
        self.img = rng.integers(0, 256, (H, W), dtype=np.uint8)
        self.pts = np.full((CAP + 8, 2), 40.0, np.float32)
        self.out = np.full((CAP + 8, 2), SENT, np.float32)   # (in/out with flags: a refused call leaves the guesses as they were)
        self.st = np.full(CAP + 8, 9, np.uint8)
        self.err = np.full(CAP + 8, SENT, np.float32)
        self.idx = np.full(CAP + 8, -5, np.int32)
        self.n_out = C.c_int(-5)
        self.pn = C.addressof(self.n_out)
        self.pointers = tuple(vp(a) for a in (self.img, self.pts, self.out, self.st, self.err, self.idx))

    def expect(self, name, want, *args):
        self.covered.add(name)
        self.checked += 1
        rc = getattr(self.lib, name)(*args)
        if rc != want:
            self.fails.append("%s%r -> %d, expected %d" % (name, tuple(str(a)[:20] for a in args[1:]), rc, want))
        elif rc < 0 and args[0] is not None and name not in self.no_message and not self.lib.vo_last_error(args[0]):
            self.fails.append("%s: vo_last_error is empty after %d" % (name, rc))
        return rc

    def untouched(self, what):
        if (self.out != SENT).any() or (self.st != 9).any() or (self.err != SENT).any() or (self.idx != -5).any() or self.n_out.value != -5:
            self.fails.append(what + " wrote to its outputs")

    def report(self):
        """closes the context, prints the JSON line; the script's exit status"""
        self.ctx.close()
        print(json.dumps({"checked": self.checked, "covered": sorted(self.covered), "failures": self.fails}))
        return 1 if self.fails else 0
