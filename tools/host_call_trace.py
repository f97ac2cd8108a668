"""Deterministic driver for a call-for-call comparison of two builds of the library's host layer: every schedule knob
pinned, every loop at most 8 steps (below the step count from which seq_enqueue_inputs consults event timings).
Library: VO_HIP_LIB or the tree's.  Writes a digest of every result to argv[1].

    VO_HIP_LIB=<build A> rocprofv3 --hip-trace --kernel-trace --memory-copy-trace -f csv -d A -o t -- python tools/host_call_trace.py A.json
    VO_HIP_LIB=<build B> rocprofv3 --hip-trace --kernel-trace --memory-copy-trace -f csv -d B -o t -- python tools/host_call_trace.py B.json
    cmp A.json B.json && python tools/host_call_trace_compare.py A B"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from visual_odom_amd import _lib as vo, synth  # noqa: E402

out = {}


def dig(*arrays):
    h = hashlib.sha1()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


W, H = 480, 160
world = synth.StereoWorld(seed=11, width=W, height=H, fx=300.0, cx=239.5, cy=79.5, bf=-160.0, tex_size=1024)
N = 9
L, R, poses, _ = world.render_sequence(N)
P_l, P_r = world.proj_matrices()
pts = synth.select_keypoints(L[0], bucket=16, per_bucket=2)
pts1 = synth.select_keypoints(L[1], bucket=16, per_bucket=2)
hip = C.CDLL("libamdhip64.so.7") if os.path.exists("/opt/rocm/lib/libamdhip64.so.7") else C.CDLL("/opt/rocm/lib/libamdhip64.so")

# ---- batch ----
for waves, streams, wide in ((2, 1, 4), (1, 2, 4)):
    ctx = vo.Context(0, W, H, 4096, 4)
    ctx.set_schedule(waves, streams, 0, wide)
    ctx.batch_configure(6, W, H, 4)
    for k in range(3):
        ctx.batch_upload_image(2 * k, L[k])
        ctx.batch_upload_image(2 * k + 1, R[k])
    ctx.batch_set_quads([[0, 1, 2, 3], [2, 3, 4, 5], [2, 3, 0, 1], [4, 5, 2, 3]])
    ctx.batch_set_projection(P_l, P_r)
    for f in range(4):
        ctx.batch_set_points(f, pts if f in (0, 3) else pts1)
    for _ in range(3):
        ctx.batch_run(vo.STAGE_ALL)
    ctx.batch_run_timed(vo.STAGE_ALL)
    ctx.batch_sync()
    res = [ctx.batch_get_pose(f) for f in range(4)]
    out["batch_%d%d" % (waves, streams)] = dig(*[r["rvec"] for r in res], *[r["tvec"] for r in res])
    for f in range(4):
        ctx.batch_set_features(f, np.zeros((0, 2), np.float32), np.zeros(0, np.int32))
    ctx.batch_set_detect_params(features_per_bucket=2)
    for st in (vo.STAGE_ALL | vo.STAGE_DETECT, vo.STAGE_ALL, vo.STAGE_ALL | vo.STAGE_DETECT):
        ctx.batch_run(st)
    ctx.batch_sync()
    res = [ctx.batch_get_pose(f) for f in range(4)]
    out["batch_det_%d%d" % (waves, streams)] = dig(*[r["rvec"] for r in res], *[r["tvec"] for r in res])
    ctx.close()

# ---- vo_track_frame: four images, then on the kept pair; mono_rotation off / on ----
for mono in (0, 1):
    ctx = vo.Context(0, W, H, 4096, 1)
    ctx.set_params(mono_rotation=mono)
    ctx.set_schedule(2, 1, 0, 4)
    g = [ctx.track_frame(L[0], R[0], L[1], R[1], pts, P_l, P_r)]
    g.append(ctx.track_frame(None, None, L[2], R[2], pts1, P_l, P_r))
    g.append(ctx.track_frame(None, None, L[3], R[3], pts1, P_l, P_r))
    g.append(ctx.track_frame(L[0], R[0], L[1], R[1], pts, P_l, P_r))
    out["track_mono%d" % mono] = dig(*[x["rvec"] for x in g], *[x["tvec"] for x in g], *[x["l1"] for x in g])
    ctx.close()


# ---- lock-step loop ----
def pinned(img):
    p = C.c_void_p()
    assert hip.hipHostMalloc(C.byref(p), C.c_size_t(img.size), 0) == 0
    v = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(img.size,)).reshape(img.shape)
    v[...] = img
    return v, p


def device(img):
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), C.c_size_t(img.size)) == 0
    assert hip.hipMemcpy(p, img.ctypes.data_as(C.c_void_p), C.c_size_t(img.size), 1) == 0
    return p


pin = [(pinned(L[k]), pinned(R[k])) for k in range(N)]
dev = [(device(L[k]), device(R[k])) for k in range(N)]
for S in (2, 40):
    ctx = vo.Context(0, W, H, 4096, S)
    ids = list(range(S))
    for prep in (0, 1):
        for streams in (1, 2):
            for kind in (0, 1, 2):
                mono = 1 if (S == 2 and prep == 1 and streams == 1 and kind == 2) else 0
                ctx.set_params(mono_rotation=mono)
                ctx.set_schedule(2 if S == 40 else 1, streams, prep, 4)
                ctx.seq_configure(S, W, H, ring=2 if kind == 1 else 3, max_steps=32)
                ctx.batch_set_projection(P_l, P_r)
                for k in range(8):
                    if kind == 0:
                        tab = ctx.seq_pair_table(ids, [L[k].ctypes.data] * S, [R[k].ctypes.data] * S)
                    elif kind == 1:
                        tab = ctx.seq_pair_table(ids, [pin[k][0][1].value] * S, [pin[k][1][1].value] * S)
                    else:
                        tab = ctx.seq_pair_table(ids, [dev[k][0].value] * S, [dev[k][1].value] * S)
                    if k == 5:  # one sequence pauses, the others go on
                        tab = ctx.seq_pair_table(ids[1:], list(tab[2])[1:], list(tab[3])[1:])
                    ctx.seq_push_pairs(tab, W, kind)
                    ctx.seq_step()
                    if k == 3:
                        ctx.seq_get_trajectory(0)  # vo_seq_sync in mid-loop
                    if k == 4 and kind == 2:  # the ingest moves to the other stream in mid-loop, and back
                        ctx.set_schedule(2 if S == 40 else 1, streams, 1 - prep, 4)
                    if k == 6 and kind == 2:
                        ctx.set_schedule(2 if S == 40 else 1, streams, prep, 4)
                tr = [ctx.seq_get_trajectory(s)[0] for s in (0, S - 1)]
                st = ctx.seq_get_state(S - 1)
                out["seq_S%d_p%d_s%d_k%d" % (S, prep, streams, kind)] = dig(*tr, st[0], st[1], st[2])
                assert ctx.get_schedule()["probed"] == 0, ctx.get_schedule()
                if kind == 0:  # start over on the same configuration
                    ctx.seq_reset(-1)
                    for k in range(3):
                        tab = ctx.seq_pair_table(ids, [L[k].ctypes.data] * S, [R[k].ctypes.data] * S)
                        ctx.seq_push_pairs(tab, W, 0)
                        ctx.seq_step()
                    out["seq_S%d_p%d_s%d_again" % (S, prep, streams)] = dig(ctx.seq_get_trajectory(0)[0])
    ctx.close()

with open(sys.argv[1], "w") as f:
    json.dump(out, f, indent=1, sort_keys=True)
print("driver ok:", len(out), "digests")
