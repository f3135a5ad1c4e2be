"""The stream promise of include/squigly_shutter.h: sq_shutter_rays_device and sq_shutter_render_device, dense and listed, only
enqueue on the caller's stream, held on the gated non-blocking side stream of tests/stream_harness.py.

A module of its own, named to run after tests/test_gpu_streams.py and the two lens modules beside it, for the reason
tests/test_gpu_streams_lens.py gives: the rig's streams come from the process's pool, and test_gpu_streams.py's control depends on
how many streams were made before it."""
import ctypes as C
import importlib

import numpy as np
import pytest

import depth_restatement as DR
import lens_restatement as LR
import mlens_restatement as MR
import shutter_restatement as SHR
import stream_harness as SH
from bitcmp import nan_eq

pytestmark = pytest.mark.gpu
f32 = np.float32
W, H, S = SHR.W, SHR.H, SHR.S
P = W * H
R = 8


def test_shutter_calls_on_a_gated_non_blocking_stream(sqt, O):
    """(1) shutter_rays: the dense call, and the listed one whose list arrives behind the gate.  (2) render_shutter: one call in three
    batches, and a sub-ray range whose carried sums arrive behind the gate.  (3) render_shutter_masked: the whole range for a list that
    arrives behind the gate.  Inputs poisoned until the gate opens (a poisoned list names no pixel), outputs poisoned behind it, the
    host arguments (motion, lens) overwritten as soon as a call returns.  Expected values are the null-stream calls', which are the
    restatement's."""
    import torch
    lens_mod = importlib.import_module("squigly-trace_amd.lens")
    shutter = importlib.import_module("squigly-trace_amd.shutter")
    L = shutter.lib()
    bright = DR.case("bright")
    env = SH.Env(sqt, torch, O, bright.bih, bright.ob)
    try:
        env.set_options(env.ds)
        lens_values = LR.LENSES["both"]
        new_motion = lambda: sqt.Motion(SHR.OPEN, SHR.CLOSE, 1.0)  # noqa: E731
        sh, rows = env.shard(W, (None, 0, 1))
        rng = np.random.default_rng(23)
        live = MR.live_list((rng.random(P) < 0.3).astype(np.uint8), None, 0)
        n1 = len(live)
        nbytes = lens_mod.work_bytes(P, 3)
        assert lens_mod.plan(P, 0, R, nbytes) == [(0, 3), (3, 6), (6, 8)]
        work = torch.empty(nbytes, dtype=torch.uint8, device=env.dev)
        first = env.ds.render_shutter(new_motion(), sqt.Lens(*lens_values), S, R, W, H, r_range=(0, 3), want_sum2=True)
        torch.cuda.synchronize()
        shape = (rows, H, 3)
        bufs = [("org", "out", ((R, P, 3), f32)), ("dir", "out", ((R, P, 3), f32)), ("seed", "out", ((R, P), np.int64)),
                ("list", "in", live), ("orgL", "out", ((2, n1, 3), f32)), ("dirL", "out", ((2, n1, 3), f32)), ("seedL", "out", ((2, n1), np.int64)),
                ("sum", "out", (shape, f32)), ("sum2", "out", (shape, f32)), ("avg", "out", (shape, f32)), ("rgb", "out", (shape, np.uint8)),
                ("carry", "inout", first.sum.cpu().numpy()), ("carry2", "inout", first.sum2.cpu().numpy()),
                ("avgB", "out", (shape, f32)), ("rgbB", "out", (shape, np.uint8)),
                ("sumM", "out", (shape, f32)), ("sum2M", "out", (shape, f32)), ("countM", "out", ((rows, H), np.int32)),
                ("avgM", "out", (shape, f32)), ("rgbM", "out", (shape, np.uint8))]

        def step_rays(B, sp, called):
            m, lens = new_motion(), sqt.Lens(*lens_values)
            shutter.check(L.sq_shutter_rays_device(0, C.byref(m), C.byref(lens), S, R, 0, R, W, H, sh, None, 0, B["org"].data_ptr(), B["dir"].data_ptr(),
                                                   B["seed"].data_ptr(), sp))
            called(m, lens)
            m, lens = new_motion(), sqt.Lens(*lens_values)
            shutter.check(L.sq_shutter_rays_device(0, C.byref(m), C.byref(lens), S, R, 5, 7, W, H, sh, B["list"].data_ptr(), n1, B["orgL"].data_ptr(),
                                                   B["dirL"].data_ptr(), B["seedL"].data_ptr(), sp))
            called(m, lens)

        def step_frames(B, sp, called):
            for r0, r1, names in ((0, R, ("sum", "sum2", "avg", "rgb")), (3, R, ("carry", "carry2", "avgB", "rgbB"))):
                m, lens = new_motion(), sqt.Lens(*lens_values)
                a = [B[n].data_ptr() for n in names]
                shutter.check(L.sq_shutter_render_device(env.ds._h, C.byref(m), C.byref(lens), S, R, r0, r1, W, H, sh, None, 0, work.data_ptr(), nbytes,
                                                         a[0], a[1], None, a[2], a[3], sp))
                called(m, lens)

        def step_masked(B, sp, called):
            m, lens = new_motion(), sqt.Lens(*lens_values)
            shutter.check(L.sq_shutter_render_device(env.ds._h, C.byref(m), C.byref(lens), S, R, 0, R, W, H, sh, B["list"].data_ptr(), n1, work.data_ptr(),
                                                     nbytes, *(B[k].data_ptr() for k in ("sumM", "sum2M", "countM", "avgM", "rgbM")), sp))
            called(m, lens)
        want = SH.drive(env, (bufs, [step_rays, step_frames, step_masked]), env.side, "shutter calls")
        # (1) the restatement's rays, dense and through the list
        ro, rd, rs = SHR.room_rays("both", R, 1.0)
        assert nan_eq(want["org"], ro).all() and nan_eq(want["dir"], rd).all() and np.array_equal(want["seed"], rs)
        assert nan_eq(want["orgL"], ro[5:7][:, live]).all() and nan_eq(want["dirL"], rd[5:7][:, live]).all() and np.array_equal(want["seedL"], rs[5:7][:, live])
        # (2) the restatement's frame, whole and carried
        for a, b in (("sum", "carry"), ("sum2", "carry2"), ("avg", "avgB"), ("rgb", "rgbB")):
            assert SH.same_result(want[a], want[b]), (a, b)
        parts = LR.sub_ray_sums(SHR.room_trails("both", R, 1.0), 3)
        s, q, avg = LR.fold(parts, S)
        assert nan_eq(want["sum"].reshape(-1, 3), s).all() and nan_eq(want["sum2"].reshape(-1, 3), q).all()
        assert np.array_equal(want["rgb"].reshape(-1, 3), LR.tonemap(avg)) and (s != 0).any(-1).sum() > 100
        # (3) the listed pixels are the dense frame's; every other pixel keeps the poison
        for name in ("sum", "sum2", "avg", "rgb"):
            assert SH.same_result(want[name + "M"].reshape(P, 3)[live], want[name].reshape(P, 3)[live]), name
        dead = np.ones(P, bool)
        dead[live] = False
        assert (want["countM"].reshape(-1)[live] == R).all() and (want["countM"].reshape(-1)[dead] == SH.POISON_OUT["int32"]).all()
        assert (want["rgbM"].reshape(P, 3)[dead] == SH.POISON_OUT["uint8"]).all() and (want["sumM"].reshape(P, 3)[dead] == SH.POISON_OUT["float32"]).all()
    finally:
        env.close()
