"""The stream promise of include/squigly_denoise.h for the glare call: sq_denoise_glare_device only enqueues on the caller's stream, and so
do denoise.glare and sqt.Film with a glare on top of it, held on the gated non-blocking side stream of tests/stream_harness.py.

A module of its own, named to run after tests/test_gpu_streams.py and the modules beside it, for the reason
tests/test_gpu_streams_lens.py gives: the rig's streams come from the process's pool, and test_gpu_streams.py's control depends on
how many streams were made before it."""
import ctypes as C
import importlib

import numpy as np
import pytest

import film_restatement as FR
import glare_restatement as R
import stream_harness as SH
from bitcmp import same

pytestmark = pytest.mark.gpu
f32 = np.float32
ROWS, COLS = 37, 70
LEVELS = 4
SETTINGS = dict(gain=(1.5, 1.0, 0.6), threshold=0.5, ceiling=8.0, spread=0.6, strength=0.3)
E = 0.7
METER = dict(key=0.18, permille=500, e_min=2.0 ** -10, e_max=2.0 ** 10, rate=0.5, fallback=1.0)


def test_glare_calls_on_a_gated_non_blocking_stream(sqt, O, product_scene, oracle_scene):
    """(1) sq_denoise_glare_device under a device exposure in both forms, and in place: the frame and the exposure arrive behind the
    gate, the results and the workspace are poisoned behind it, and the host struct is overwritten as soon as each call returns.
    (2) denoise.glare, which allocates its result and workspace under the stream, and sqt.Film with auto-exposure, glare and balance.
    Expected values are the null-stream calls'; all are the restatement's."""
    import torch
    dn = importlib.import_module("squigly-trace_amd.denoise")
    env = SH.Env(sqt, torch, O, product_scene[0], oracle_scene[0])
    try:
        px = R.random_frame(ROWS, COLS, 41)
        need = R.work_bytes(ROWS, COLS, LEVELS)
        bufs = [("color", "in", px), ("e", "in", np.array([E], f32)), ("same", "inout", px),
                ("direct", "out", (px.shape, f32)), ("tiled", "out", (px.shape, f32)), ("work", "out", ((need // 4,), f32)),
                ("d_out", "out", (px.shape, f32)), ("f_rgb", "out", (px.shape, np.uint8)), ("f_state", "out", ((1,), f32))]
        L = dn.lib()
        film = sqt.Film(curve="filmic", auto=METER, glare=sqt.Glare(levels=LEVELS, **{k: v for k, v in SETTINGS.items() if k != "gain"}),
                        balance=SETTINGS["gain"])

        def step_calls(B, sp, called):
            p = lambda n: B[n].data_ptr()                                                  # noqa: E731
            for form, src, out in ((1, "color", "direct"), (2, "color", "tiled"), (0, "same", "same")):
                P = dn.make_glare_params(-5.0, levels=LEVELS, form=form, **SETTINGS)           # exposure: not read, d_exposure is given
                dn.check(L.sq_denoise_glare_device(0, ROWS, COLS, p(src), p("e"), C.byref(P), p(out), p("work"), need, sp))
                called(P)

        def step_driver(B, sp, called):
            st = env.side if sp is not None else None
            film.reset()
            with torch.cuda.stream(st if st is not None else torch.cuda.current_stream()):
                out = dn.glare(B["color"], exposure=B["e"], levels=LEVELS, stream=st, **SETTINGS)
                called()
                B["d_out"].copy_(out)
                rgb = film(B["color"], stream=st)
                called()
                B["f_rgb"].copy_(rgb)
                B["f_state"].copy_(film._state)

        want = SH.drive(env, (bufs, [step_calls, step_driver]), env.side, "glare calls")
        x = R.glare(px, E, levels=LEVELS, **SETTINGS)
        assert same(want["direct"], x) and same(want["tiled"], x) and same(want["same"], x) and same(want["d_out"], x)
        e0 = FR.expose(FR.histogram(px), None, **METER)
        assert same(want["f_state"], np.array([e0], f32))
        assert np.array_equal(want["f_rgb"], FR.develop(O, R.glare(px, e0, levels=LEVELS, **SETTINGS), 1.0, "filmic")[0])
    finally:
        env.close()
