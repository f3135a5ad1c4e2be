"""The stream promise of include/squigly_lens.h: sq_lens_render_device only enqueues on the caller's stream, held on the gated
non-blocking side stream of tests/stream_harness.py.

A module of its own, named to run after tests/test_gpu_streams.py: the rig's streams come from the process's pool, and that module's
control -- a gate on a side stream must not hold back the null stream -- depends on which of them it is handed, that is on how many
streams were made before it."""
import ctypes as C
import importlib

import numpy as np
import pytest

import depth_restatement as DR
import lens_restatement as LR
import stream_harness as SH
from bitcmp import nan_eq

pytestmark = pytest.mark.gpu
f32 = np.float32
W, H, S = LR.W, LR.H, LR.S
P = W * H


def test_render_lens_on_a_gated_non_blocking_stream(sqt, O):
    """One sq_lens_render_device call -- three batches -- and one sub-ray range whose carried sums arrive behind the gate: inputs
    poisoned until the gate opens, outputs poisoned behind it, the host arguments (camera, lens) overwritten as soon as the call
    returns.  Expected values are the null-stream call's, which is the restatement's frame."""
    import torch
    lens_mod = importlib.import_module("squigly-trace_amd.lens")
    L = lens_mod.lib()
    bright = DR.case("bright")
    env = SH.Env(sqt, torch, O, bright.bih, bright.ob)
    try:
        env.set_options(env.ds)
        lens_values = LR.LENSES["both"]
        sh, rows = env.shard(W, (None, 0, 1))
        nbytes = lens_mod.work_bytes(P, 3)
        assert lens_mod.plan(P, 0, 8, nbytes) == [(0, 3), (3, 6), (6, 8)]
        work = torch.empty(nbytes, dtype=torch.uint8, device=env.dev)
        first = env.ds.render_lens(env.new_cam(), sqt.Lens(*lens_values), S, 8, W, H, r_range=(0, 3), want_sum2=True)
        torch.cuda.synchronize()
        shape = (rows, H, 3)
        bufs = [("sum", "out", (shape, f32)), ("sum2", "out", (shape, f32)), ("avg", "out", (shape, f32)), ("rgb", "out", (shape, np.uint8)),
                ("carry", "inout", first.sum.cpu().numpy()), ("carry2", "inout", first.sum2.cpu().numpy()),
                ("avgB", "out", (shape, f32)), ("rgbB", "out", (shape, np.uint8))]

        def step(B, sp, called):
            for r0, r1, names in ((0, 8, ("sum", "sum2", "avg", "rgb")), (3, 8, ("carry", "carry2", "avgB", "rgbB"))):
                cam, lens = env.new_cam(), sqt.Lens(*lens_values)
                lens_mod.check(L.sq_lens_render_device(env.ds._h, C.byref(cam), C.byref(lens), S, 8, r0, r1, W, H, sh, work.data_ptr(), nbytes,
                                                       *(B[n].data_ptr() for n in names), sp))
                called(cam, lens)
        want = SH.drive(env, (bufs, [step]), env.side, "lens frame")
        for a, b in (("sum", "carry"), ("sum2", "carry2"), ("avg", "avgB"), ("rgb", "rgbB")):
            assert SH.same_result(want[a], want[b]), (a, b)
        parts = LR.sub_ray_sums(LR.room_trails("both", 8), 3)
        s, q, avg = LR.fold(parts, S)
        assert nan_eq(want["sum"].reshape(-1, 3), s).all() and nan_eq(want["sum2"].reshape(-1, 3), q).all()
        assert np.array_equal(want["rgb"].reshape(-1, 3), LR.tonemap(avg)) and (s != 0).any(-1).sum() > 100
    finally:
        env.close()
