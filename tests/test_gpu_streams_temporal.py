"""The stream promise of include/squigly_temporal.h: accumulate and unpack only enqueue on the caller's stream, and so does a step of
sqt.Temporal on top of them, held on the gated non-blocking side stream of tests/stream_harness.py.

A module of its own, named to run after tests/test_gpu_streams.py and the modules beside it, for the reason
tests/test_gpu_streams_lens.py gives: the rig's streams come from the process's pool, and test_gpu_streams.py's control depends on
how many streams were made before it."""
import collections
import ctypes as C
import importlib

import numpy as np
import pytest

import stream_harness as SH
import temporal_restatement as R
import temporal_room as TR
from bitcmp import same

pytestmark = pytest.mark.gpu
f32 = np.float32
G = collections.namedtuple("G", ["tri", "normal", "point"])
ROWS, COLS = 37, 70
SIGMA_P = 0.05
CAM = ((0, 0, 0), R.IDENTITY)
PREV_CAM = ((0.2, 0.04, -0.02), R.turned(0.01))


def test_temporal_calls_on_a_gated_non_blocking_stream(sqt, O, product_scene, oracle_scene):
    """(1) accumulate with a previous block and d_alpha, then unpack of the block it wrote: every image and the previous block arrive
    behind the gate, every output is poisoned behind it, and the host arguments (camera, parameters) are overwritten as soon as the
    call returns.  (2) A step of sqt.Temporal resumed from a history that arrives behind the gate.  Expected values are the
    null-stream calls'; those of (1) are the restatement's."""
    import torch
    tp = importlib.import_module("squigly-trace_amd.temporal")
    env = SH.Env(sqt, torch, O, product_scene[0], oracle_scene[0])
    try:
        env.set_options(env.ds)
        cur, prev = R.synthetic(ROWS, COLS, 31, CAM, 0.01), R.synthetic(ROWS, COLS, 32, PREV_CAM, 0.01)
        alpha = np.random.default_rng(33).random((ROWS, COLS)).astype(f32)
        # the previous block's bytes, from a first frame on the null stream
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()                   # noqa: E731
        pblk = tp.history(ROWS, COLS, 0)
        tp.accumulate(dev(prev[0]), dev(prev[1]), G(dev(prev[2]), dev(prev[3]), dev(prev[4])), None, None, pblk, sigma_p=SIGMA_P)
        # ... and the driver's checkpoint after one frame of the room
        spp, w, h = 4, TR.W, TR.H
        cams = [TR.CAMERA_TEXTS[0], TR.CAMERA_TEXTS[1]]
        t0 = sqt.Temporal(env.ds, w, h, spp)
        t0.step(sqt.camera_from_text(cams[0]))
        torch.cuda.synchronize()
        nbytes, tbytes = tp.history_bytes(ROWS, COLS), tp.history_bytes(w, h)
        u8 = np.uint8
        bufs = [("color", "in", cur[0]), ("var", "in", cur[1]), ("tri", "in", cur[2]), ("normal", "in", cur[3]), ("point", "in", cur[4]),
                ("alpha", "in", alpha), ("prev", "in", pblk.cpu().numpy()),
                ("next", "out", ((nbytes,), u8)), ("out", "out", ((ROWS, COLS, 3), f32)), ("out_var", "out", ((ROWS, COLS), f32)),
                ("out_len", "out", ((ROWS, COLS), np.int32)),
                ("u_color", "out", ((ROWS, COLS, 3), f32)), ("u_var", "out", ((ROWS, COLS), f32)), ("u_len", "out", ((ROWS, COLS), np.int32)),
                ("u_tri", "out", ((ROWS, COLS), np.int32)), ("u_normal", "out", ((ROWS, COLS, 3), f32)), ("u_point", "out", ((ROWS, COLS, 3), f32)),
                ("thist", "in", t0.history.cpu().numpy()),
                ("t_avg", "out", ((w, h, 3), f32)), ("t_var", "out", ((w, h), f32)), ("t_len", "out", ((w, h), np.int32)),
                ("t_rgb", "out", ((w, h, 3), u8)), ("t_next", "out", ((tbytes,), u8))]
        L = tp.lib()

        def step_calls(B, sp, called):
            cam = sqt.Camera()
            pos, rot = R.camera(PREV_CAM)
            cam.pos[:], cam.rot[:] = [float(v) for v in pos], [float(v) for v in rot]
            P = tp.make_params(sigma_p=SIGMA_P)
            p = lambda n: B[n].data_ptr()                                                  # noqa: E731
            tp.check(L.sq_temporal_accumulate_device(0, ROWS, COLS, p("color"), p("var"), p("tri"), p("normal"), p("point"), p("alpha"),
                                                     C.byref(cam), p("prev"), C.byref(P), p("next"), p("out"), p("out_var"), p("out_len"), sp))
            called(cam, P)
            tp.check(L.sq_temporal_unpack_device(0, ROWS, COLS, p("next"), p("u_color"), p("u_var"), p("u_len"), p("u_tri"), p("u_normal"),
                                                 p("u_point"), sp))
            called()

        def step_driver(B, sp, called):
            st = env.side if sp is not None else None
            with torch.cuda.stream(st if st is not None else torch.cuda.current_stream()):
                prev_cam = sqt.camera_from_text(cams[0])
                t = sqt.Temporal(env.ds, w, h, spp, history=B["thist"], camera=prev_cam, frames=1)
                cam = sqt.camera_from_text(cams[1])
                avg, var, length, rgb = t.step(cam, stream=st)
                called(cam, prev_cam)
                for name, src in (("t_avg", avg), ("t_var", var), ("t_len", length), ("t_rgb", rgb), ("t_next", t.history)):
                    B[name].copy_(src)

        want = SH.drive(env, (bufs, [step_calls, step_driver]), env.side, "temporal calls")
        # (1) the restatement's
        ref = R.accumulate(*cur, PREV_CAM, R.first_block(*prev), alpha=alpha, sigma_p=SIGMA_P)
        assert same(want["out"], ref["color"]) and same(want["out_var"], ref["var"]) and np.array_equal(want["out_len"], ref["len"])
        assert (ref["len"] == 2).sum() > 1000
        for name in R.BLOCK_FIELDS:
            g, r = want["u_" + name], ref["block"][name]
            assert (same(g, r) if r.dtype == f32 else np.array_equal(g, r)), name
        # (2) the step accumulated: most hit pixels have two frames behind them, and the block it wrote holds its result
        assert (want["t_len"] == 2).sum() > 1000 and (want["t_len"] == 1).any() and want["t_rgb"].any()
        assert (want["t_next"] != SH.POISON_OUT["uint8"]).any()
    finally:
        env.close()
