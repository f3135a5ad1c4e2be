"""The stream promise of include/squigly_mlens.h: sq_mlens_live_device and sq_mlens_render_device only enqueue on the caller's
stream, held on the gated non-blocking side stream of tests/stream_harness.py.

A module of its own, named to run after tests/test_gpu_streams.py and tests/test_gpu_streams_lens.py, for the reason the latter
gives: the rig's streams come from the process's pool, and test_gpu_streams.py's control depends on how many streams were made
before it."""
import ctypes as C
import importlib

import numpy as np
import pytest

import depth_restatement as DR
import lens_restatement as LR
import mlens_restatement as MR
import stream_harness as SH
from bitcmp import nan_eq

pytestmark = pytest.mark.gpu
f32 = np.float32
W, H, P = MR.W, MR.H, MR.P
S, R = LR.S, 8


def test_masked_lens_step_on_a_gated_non_blocking_stream(sqt, O):
    """Two steps.  (1) The live-list call, then the range [3, 8) for its list in three batches: mask, counts and the carried sums
    arrive behind the gate, and so does the list, which the first call writes there.  (2) The whole range for a list that is an
    input and arrives behind the gate.  Inputs poisoned until the gate opens (a poisoned list names no pixel), outputs poisoned
    behind it, the host arguments (camera, lens) overwritten as soon as a call returns.  Expected values are the null-stream calls',
    which are the restatement's."""
    import torch
    lens_mod = importlib.import_module("squigly-trace_amd.lens")
    mlens = importlib.import_module("squigly-trace_amd.mlens")
    L = mlens.lib()
    bright = DR.case("bright")
    env = SH.Env(sqt, torch, O, bright.bih, bright.ob)
    try:
        env.set_options(env.ds)
        lens_values = LR.LENSES["both"]
        sh, rows = env.shard(W, (None, 0, 1))
        rng = np.random.default_rng(17)
        mask1 = (rng.random((rows, H)) < 0.3).astype(np.uint8)
        mask2 = mask1 & (rng.random((rows, H)) < 0.5).astype(np.uint8)
        list1 = MR.live_list(mask1.reshape(-1), None, 0)
        n1, n2 = len(list1), int(mask2.sum())
        # the state after the sub-rays [0, 3) of mask1, from the null stream
        st = {k: torch.full(shape, v, dtype=dt, device=env.dev) for k, shape, v, dt in
              (("sums", (rows, H, 3), 7.25, torch.float32), ("sums2", (rows, H, 3), 5.5, torch.float32), ("counts", (rows, H), 77, torch.int32),
               ("avg", (rows, H, 3), -3.5, torch.float32), ("rgb", (rows, H, 3), 123, torch.uint8))}
        index, n_live = env.ds.live_pixels(torch.from_numpy(mask1).to(env.dev), st["counts"], 0)
        assert int(n_live.item()) == n1
        env.ds.render_lens_masked(env.new_cam(), sqt.Lens(*lens_values), S, R, W, H, 0, 3, st["sums"], index, n1, sums2=st["sums2"],
                                  counts=st["counts"], out_avg=st["avg"], out_rgb=st["rgb"])
        torch.cuda.synchronize()
        nbytes = lens_mod.work_bytes(n2, 2)
        assert lens_mod.plan(n2, 3, 8, nbytes) == [(3, 5), (5, 7), (7, 8)]
        work = torch.empty(max(nbytes, lens_mod.work_bytes(n1, 8)), dtype=torch.uint8, device=env.dev)
        shape = (rows, H, 3)
        bufs = [("mask", "in", mask2)] + [(k, "inout", st[k].cpu().numpy()) for k in ("sums", "sums2", "counts", "avg", "rgb")] + \
               [("index", "out", ((P,), np.int32)), ("n_live", "out", ((1,), np.int32)),
                ("listB", "in", list1), ("sumB", "out", (shape, f32)), ("sum2B", "out", (shape, f32)), ("countB", "out", ((rows, H), np.int32)),
                ("avgB", "out", (shape, f32)), ("rgbB", "out", (shape, np.uint8))]

        def step_a(B, sp, called):
            mlens.check(L.sq_mlens_live_device(0, P, 3, B["mask"].data_ptr(), B["counts"].data_ptr(), B["index"].data_ptr(), B["n_live"].data_ptr(), sp))
            called()
            cam, lens = env.new_cam(), sqt.Lens(*lens_values)
            mlens.check(L.sq_mlens_render_device(env.ds._h, C.byref(cam), C.byref(lens), S, R, 3, 8, W, H, sh, B["index"].data_ptr(), n2, work.data_ptr(),
                                                 nbytes, *(B[k].data_ptr() for k in ("sums", "sums2", "counts", "avg", "rgb")), sp))
            called(cam, lens)

        def step_b(B, sp, called):
            cam, lens = env.new_cam(), sqt.Lens(*lens_values)
            mlens.check(L.sq_mlens_render_device(env.ds._h, C.byref(cam), C.byref(lens), S, R, 0, 8, W, H, sh, B["listB"].data_ptr(), n1, work.data_ptr(),
                                                 work.numel(), *(B[k].data_ptr() for k in ("sumB", "sum2B", "countB", "avgB", "rgbB")), sp))
            called(cam, lens)
        want = SH.drive(env, (bufs, [step_a, step_b]), env.side, "masked lens step")
        # (1): the list of mask2 among the pixels at 3 sub-rays, its length, and the restatement's state
        list2 = MR.live_list(mask2.reshape(-1), st["counts"].cpu().numpy().reshape(-1), 3)
        assert len(list2) == n2 and int(want["n_live"][0]) == n2 and np.array_equal(want["index"][:n2], list2)
        assert (want["index"][n2:] == SH.POISON_OUT["int32"]).all()
        parts = MR.sub_ray_sums("both", S, R)
        ref = {"sum": np.full((P, 3), 7.25, f32), "sum2": np.full((P, 3), 5.5, f32), "count": np.full(P, 77, np.int32),
               "avg": np.full((P, 3), -3.5, f32), "rgb": np.full((P, 3), 123, np.uint8)}
        MR.indexed_fold(parts[0:3][:, list1], list1, S // R, 0, 3, ref)
        MR.indexed_fold(parts[3:8][:, list2], list2, S // R, 3, 8, ref)
        for k, name in (("sum", "sums"), ("sum2", "sums2"), ("avg", "avg")):
            assert nan_eq(want[name].reshape(-1, 3), ref[k]).all(), name
        assert np.array_equal(want["counts"].reshape(-1), ref["count"]) and np.array_equal(want["rgb"].reshape(-1, 3), ref["rgb"])
        assert (ref["sum"][list2] != 0).any(-1).sum() > 20
        # (2): the whole range for the pixels of mask1; every other pixel keeps the poison
        whole = MR.indexed_fold(parts[:, list1], list1, S // R, 0, 8, {"sum": np.zeros((P, 3), f32), "sum2": np.zeros((P, 3), f32),
                                                                        "count": np.zeros(P, np.int32), "rgb": np.zeros((P, 3), np.uint8)})
        assert nan_eq(want["sumB"].reshape(-1, 3)[list1], whole["sum"][list1]).all() and nan_eq(want["sum2B"].reshape(-1, 3)[list1], whole["sum2"][list1]).all()
        assert np.array_equal(want["rgbB"].reshape(-1, 3)[list1], whole["rgb"][list1]) and (want["countB"].reshape(-1)[list1] == 8).all()
        dead = mask1.reshape(-1) == 0
        assert (want["countB"].reshape(-1)[dead] == SH.POISON_OUT["int32"]).all() and (want["rgbB"].reshape(-1, 3)[dead] == SH.POISON_OUT["uint8"]).all()
    finally:
        env.close()
