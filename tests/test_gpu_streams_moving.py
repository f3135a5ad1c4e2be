"""The stream promise of include/squigly_temporal.h for sq_temporal_accumulate_moving_device, and for a step of sqt.Temporal on a
scene of its own with a move and a clamp, held on the gated non-blocking side stream of tests/stream_harness.py.

A module of its own, named to run after tests/test_gpu_streams.py and the modules beside it, for the reason
tests/test_gpu_streams_lens.py gives: the rig's streams come from the process's pool, and test_gpu_streams.py's control depends on
how many streams were made before it."""
import ctypes as C
import importlib

import numpy as np
import pytest

import moving_restatement as M
import moving_room as MR
import stream_harness as SH
import temporal_restatement as R
from bitcmp import same

pytestmark = pytest.mark.gpu
f32 = np.float32
ROWS, COLS = 37, 70
SIGMA_P = 0.05
N_TRIS = 21
CAM = ((0, 0, 0), R.IDENTITY)
PREV_CAM = ((0.2, 0.04, -0.02), R.turned(0.01))
CLAMP = (2, 1.0)                         # (radius, k)


def test_moving_calls_on_a_gated_non_blocking_stream(sqt, O, product_scene, oracle_scene):
    """(1) The moving call with a previous block, d_alpha, both tables, a clamp and flags, in both kernel forms: every image, the
    previous block and the two tables arrive behind the gate, every output is poisoned behind it, and the host arguments (camera,
    parameters, clamp) are overwritten as soon as the call returns.  (2) A step of sqt.Temporal on the second frame's scene of the
    moving room, with the box's move and a clamp, resumed from a history that arrives behind the gate.  Expected values are the
    null-stream calls'; those of (1) are the restatement's."""
    import torch
    tp = importlib.import_module("squigly-trace_amd.temporal")
    env = SH.Env(sqt, torch, O, product_scene[0], oracle_scene[0])
    mesh, poses, box = MR.product_mesh(sqt, product_scene[2])
    scenes = [sqt.DeviceScene(sqt.BIH(sqt.moved_mesh(mesh, poses[f])), 0) for f in range(2)]
    try:
        env.set_options(env.ds)
        cur, prev = R.synthetic(ROWS, COLS, 31, CAM, 0.01), R.synthetic(ROWS, COLS, 32, PREV_CAM, 0.01)
        M.scatter_triangles(cur[2], N_TRIS, 33)
        alpha = np.random.default_rng(33).random((ROWS, COLS)).astype(f32)
        objects, back = M.tables(N_TRIS, 0)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()                   # noqa: E731
        G = importlib.import_module("collections").namedtuple("G", ["tri", "normal", "point"])
        pblk = tp.history(ROWS, COLS, 0)
        tp.accumulate(dev(prev[0]), dev(prev[1]), G(dev(prev[2]), dev(prev[3]), dev(prev[4])), None, None, pblk, sigma_p=SIGMA_P)
        # ... and the driver's checkpoint after the first frame of the moving room
        spp, w, h = 4, MR.W, MR.H
        cam_text = MR.CAMERA_TEXT
        t0 = sqt.Temporal(scenes[0], w, h, spp, clamp=(1.0, 2))
        t0.step(sqt.camera_from_text(cam_text), scene=scenes[0])
        move = tp.back_transforms(poses[0], poses[1])
        for ds in scenes:
            tp.object_table(ds), tp.alpha_table(ds)                                        # built once per scene, before the gate
        torch.cuda.synchronize()
        nbytes, tbytes = tp.history_bytes(ROWS, COLS), tp.history_bytes(w, h)
        u8 = np.uint8
        bufs = [("color", "in", cur[0]), ("var", "in", cur[1]), ("tri", "in", cur[2]), ("normal", "in", cur[3]), ("point", "in", cur[4]),
                ("alpha", "in", alpha), ("prev", "in", pblk.cpu().numpy()), ("object", "in", objects), ("back", "in", back.reshape(-1))]
        for form in ("d", "t"):
            bufs += [(form + "next", "out", ((nbytes,), u8)), (form + "out", "out", ((ROWS, COLS, 3), f32)),
                     (form + "out_var", "out", ((ROWS, COLS), f32)), (form + "out_len", "out", ((ROWS, COLS), np.int32)),
                     (form + "flags", "out", ((ROWS, COLS), u8))]
        bufs += [("thist", "in", t0.history.cpu().numpy()),
                 ("t_avg", "out", ((w, h, 3), f32)), ("t_var", "out", ((w, h), f32)), ("t_len", "out", ((w, h), np.int32)),
                 ("t_rgb", "out", ((w, h, 3), u8)), ("t_next", "out", ((tbytes,), u8)), ("t_flags", "out", ((w, h), u8))]
        L = tp.lib()

        def step_calls(B, sp, called):
            p = lambda n: B[n].data_ptr()                                                  # noqa: E731
            for form, code in (("d", tp.FORMS["direct"]), ("t", tp.FORMS["tiled"])):
                cam = sqt.Camera()
                pos, rot = R.camera(PREV_CAM)
                cam.pos[:], cam.rot[:] = [float(v) for v in pos], [float(v) for v in rot]
                P, K = tp.make_params(sigma_p=SIGMA_P), tp.Clamp(*CLAMP)
                tp.check(L.sq_temporal_accumulate_moving_device(
                    0, ROWS, COLS, p("color"), p("var"), p("tri"), p("normal"), p("point"), p("alpha"), C.byref(cam), p("prev"), C.byref(P),
                    p("object"), N_TRIS, p("back"), len(back), C.byref(K), code, p(form + "next"), p(form + "out"), p(form + "out_var"),
                    p(form + "out_len"), p(form + "flags"), sp))
                called(cam, P, K)

        def step_driver(B, sp, called):
            st = env.side if sp is not None else None
            with torch.cuda.stream(st if st is not None else torch.cuda.current_stream()):
                prev_cam = sqt.camera_from_text(cam_text)
                t = sqt.Temporal(scenes[0], w, h, spp, history=B["thist"], camera=prev_cam, frames=1, clamp=(1.0, 2))
                cam, mv = sqt.camera_from_text(cam_text), move.copy()
                avg, var, length, rgb = t.step(cam, stream=st, scene=scenes[1], back=mv)
                called(cam, prev_cam, mv)
                for name, src in (("t_avg", avg), ("t_var", var), ("t_len", length), ("t_rgb", rgb), ("t_next", t.history), ("t_flags", t.flags)):
                    B[name].copy_(src)

        want = SH.drive(env, (bufs, [step_calls, step_driver]), env.side, "moving calls")
        # (1) the restatement's, in both forms
        ref = M.accumulate(*cur, PREV_CAM, R.first_block(*prev), alpha=alpha, objects=objects, back=back, clamp=CLAMP, sigma_p=SIGMA_P)
        for form in ("d", "t"):
            assert same(want[form + "out"], ref["color"]) and same(want[form + "out_var"], ref["var"]), form
            assert np.array_equal(want[form + "out_len"], ref["len"]) and np.array_equal(want[form + "flags"], ref["flags"]), form
            assert np.array_equal(want[form + "next"], want["dnext"])
        seen = int(np.bitwise_or.reduce(ref["flags"].reshape(-1)))
        assert seen == M.BLENDED | M.CLAMPED | M.MOVED and (ref["len"] == 2).sum() > 500
        # (2) the step accumulated through the move
        assert (want["t_len"] == 2).sum() > 1000 and want["t_rgb"].any() and (want["t_flags"] & tp.FLAG_MOVED).any()
        assert (want["t_next"] != SH.POISON_OUT["uint8"]).any()
    finally:
        torch.cuda.synchronize()
        for ds in scenes:
            ds.close()
        env.close()
