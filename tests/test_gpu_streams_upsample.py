"""The stream promise of the sparse-frame calls of include/squigly_denoise.h: sq_denoise_sparse_mask_device and
sq_denoise_upsample_device only enqueue on the caller's stream, and so does a step of sqt.Temporal(sparse=) on top of them, held on
the gated non-blocking side stream of tests/stream_harness.py.

A module of its own, named to run after tests/test_gpu_streams.py and the modules beside it, for the reason
tests/test_gpu_streams_lens.py gives: the rig's streams come from the process's pool, and test_gpu_streams.py's control depends on
how many streams were made before it."""
import ctypes as C
import importlib

import numpy as np
import pytest

import stream_harness as SH
import temporal_room as TR
import upsample_restatement as R
from bitcmp import same

pytestmark = pytest.mark.gpu
f32 = np.float32
ROWS, COLS = 37, 70
S, OFF = 3, (2, 1)
STOPS = dict(sigma_p=0.05, cos_n=0.9)


def test_sparse_calls_on_a_gated_non_blocking_stream(sqt, O, product_scene, oracle_scene):
    """(1) The mask of guides that arrive behind the gate, then the fill under that mask of images that arrive behind it: every
    output is poisoned behind the gate, and the host struct is overwritten as soon as each call returns.  (2) A step of
    sqt.Temporal(sparse=2) resumed from a history that arrives behind the gate.  Expected values are the null-stream calls'; those of
    (1) are the restatement's."""
    import torch
    dn = importlib.import_module("squigly-trace_amd.denoise")
    env = SH.Env(sqt, torch, O, product_scene[0], oracle_scene[0])
    try:
        env.set_options(env.ds)
        color, var, tri, nrm, pnt = R.synthetic(ROWS, COLS, seed=21)
        spp, w, h = 4, TR.W, TR.H
        cams = [TR.CAMERA_TEXTS[0], TR.CAMERA_TEXTS[1]]
        t0 = sqt.Temporal(env.ds, w, h, spp, sparse=2)
        t0.step(sqt.camera_from_text(cams[0]))
        torch.cuda.synchronize()
        tp = importlib.import_module("squigly-trace_amd.temporal")
        tbytes = tp.history_bytes(w, h)
        u8 = np.uint8
        bufs = [("color", "in", color), ("var", "in", var), ("tri", "in", tri), ("normal", "in", nrm), ("point", "in", pnt),
                ("live", "out", ((ROWS, COLS), u8)), ("out", "out", ((ROWS, COLS, 3), f32)), ("out_var", "out", ((ROWS, COLS), f32)),
                ("thist", "in", t0.history.cpu().numpy()),
                ("t_avg", "out", ((w, h, 3), f32)), ("t_var", "out", ((w, h), f32)), ("t_len", "out", ((w, h), np.int32)),
                ("t_rgb", "out", ((w, h, 3), u8)), ("t_next", "out", ((tbytes,), u8)), ("t_live", "out", ((w, h), u8))]
        L = dn.lib()

        def step_calls(B, sp, called):
            p = lambda n: B[n].data_ptr()                                                  # noqa: E731
            P = dn.SparseParams(STOPS["sigma_p"], STOPS["cos_n"])
            dn.check(L.sq_denoise_sparse_mask_device(0, ROWS, COLS, S, OFF[0], OFF[1], p("tri"), p("normal"), p("point"), C.byref(P),
                                                     p("live"), sp))
            called(P)
            P = dn.SparseParams(STOPS["sigma_p"], STOPS["cos_n"])
            dn.check(L.sq_denoise_upsample_device(0, ROWS, COLS, S, OFF[0], OFF[1], p("color"), p("var"), p("tri"), p("normal"), p("point"),
                                                  p("live"), C.byref(P), p("out"), p("out_var"), sp))
            called(P)

        def step_driver(B, sp, called):
            st = env.side if sp is not None else None
            with torch.cuda.stream(st if st is not None else torch.cuda.current_stream()):
                prev_cam = sqt.camera_from_text(cams[0])
                t = sqt.Temporal(env.ds, w, h, spp, sparse=2, history=B["thist"], camera=prev_cam, frames=1)
                cam = sqt.camera_from_text(cams[1])
                avg, var_, length, rgb = t.step(cam, stream=st)
                called(cam, prev_cam)
                for name, src in (("t_avg", avg), ("t_var", var_), ("t_len", length), ("t_rgb", rgb), ("t_next", t.history), ("t_live", t.live)):
                    B[name].copy_(src)

        want = SH.drive(env, (bufs, [step_calls, step_driver]), env.side, "sparse calls")
        # (1) the restatement's
        mask = R.sparse_mask(tri, nrm, pnt, S, *OFF, **STOPS)
        ref, ref_var = R.upsample(color, tri, nrm, pnt, mask, S, *OFF, var=var, **STOPS)
        assert np.array_equal(want["live"], mask) and same(want["out"], ref) and same(want["out_var"], ref_var)
        lat = R.lattice(ROWS, COLS, S, *OFF)
        assert ((mask != 0) & ~lat).sum() > 20 and (mask == 0).sum() > 1000
        # (2) the step traced the second frame's lattice and the holes, and accumulated
        assert np.array_equal(want["t_live"][R.lattice(w, h, 2, 1, 1)], np.ones(R.lattice(w, h, 2, 1, 1).sum(), u8))
        assert 0.2 < (want["t_live"] != 0).mean() < 0.35
        assert (want["t_len"] == 2).sum() > 1000 and (want["t_len"] == 1).any() and want["t_rgb"].any()
        assert (want["t_next"] != SH.POISON_OUT["uint8"]).any()
    finally:
        env.close()
