"""The stream promise of include/squigly_film.h: histogram, expose and develop only enqueue on the caller's stream, and so does
sqt.Film with auto-exposure on top of them, held on the gated non-blocking side stream of tests/stream_harness.py.

A module of its own, named to run after tests/test_gpu_streams.py and the modules beside it, for the reason
tests/test_gpu_streams_lens.py gives: the rig's streams come from the process's pool, and test_gpu_streams.py's control depends on
how many streams were made before it."""
import ctypes as C
import importlib

import numpy as np
import pytest

import film_restatement as R
import stream_harness as SH
from bitcmp import same

pytestmark = pytest.mark.gpu
f32 = np.float32
ROWS, COLS = 37, 70
METER = dict(key=0.18, permille=500, e_min=2.0 ** -10, e_max=2.0 ** 10, rate=0.5, fallback=1.0)
PREV = 3.0


def test_film_calls_on_a_gated_non_blocking_stream(sqt, O, product_scene, oracle_scene):
    """(1) histogram, expose (with a previous exposure; then once more in place) and develop under that device exposure, with a table,
    dither and d_display: the frame, the table and the previous exposure arrive behind the gate, every output is poisoned behind it,
    and the host structs (meter, parameters) are overwritten as soon as each call returns.  (2) sqt.Film with auto-exposure over the
    same frame, its table uploaded before the gate.  Expected values are the null-stream calls'; both are the restatement's."""
    import torch
    fm = importlib.import_module("squigly-trace_amd.film")
    env = SH.Env(sqt, torch, O, product_scene[0], oracle_scene[0])
    try:
        px = R.value_table(ROWS * COLS, 41).reshape(ROWS, COLS, 3)
        table = fm.srgb_lut(256)
        u8 = np.uint8
        bufs = [("color", "in", px), ("lut", "in", table), ("prev", "in", np.array([PREV], f32)),
                ("hist", "out", ((R.SLOTS,), np.int32)), ("e", "out", ((1,), f32)), ("state", "inout", np.array([PREV], f32)),
                ("rgb", "out", (px.shape, u8)), ("display", "out", (px.shape, f32)),
                ("f_rgb", "out", (px.shape, u8)), ("f_state", "out", ((1,), f32))]
        L = fm.lib()
        film = sqt.Film(curve="filmic", lut=table, dither=True, auto=METER)
        film.prepare(0)                                                 # a constant of the film, not of a call
        torch.cuda.synchronize()

        def step_calls(B, sp, called):
            p = lambda n: B[n].data_ptr()                                                  # noqa: E731
            fm.check(L.sq_film_histogram_device(0, ROWS, COLS, p("color"), p("hist"), sp))
            called()
            for prev, out in (("prev", "e"), ("state", "state")):
                M = fm.make_meter(**METER)
                fm.check(L.sq_film_expose_device(0, p("hist"), C.byref(M), p(prev), p(out), sp))
                called(M)
            P = fm.make_params(-5.0, "filmic", n_lut=len(table), dither=True)                  # exposure: not read, d_exposure is given
            fm.check(L.sq_film_develop_device(0, ROWS, COLS, p("color"), p("e"), C.byref(P), p("lut"), p("rgb"), p("display"), sp))
            called(P)

        def step_driver(B, sp, called):
            st = env.side if sp is not None else None
            film.reset()
            with torch.cuda.stream(st if st is not None else torch.cuda.current_stream()):
                rgb = film(B["color"], stream=st)
                called()
                B["f_rgb"].copy_(rgb)
                B["f_state"].copy_(film._state)

        want = SH.drive(env, (bufs, [step_calls, step_driver]), env.side, "film calls")
        hist = R.histogram(px)
        assert np.array_equal(want["hist"].astype(np.int64), hist) and hist.sum() == ROWS * COLS
        e = R.expose(hist, PREV, **METER)
        assert same(want["e"], np.array([e], f32)) and same(want["state"], want["e"]) and e != PREV
        rgb, disp = R.develop(O, px, e, "filmic", np.inf, table, True)
        assert np.array_equal(want["rgb"], rgb) and same(want["display"], disp)
        e0 = R.expose(hist, None, **METER)
        assert same(want["f_state"], np.array([e0], f32)) and np.array_equal(want["f_rgb"], R.develop(O, px, e0, "filmic", np.inf, table, True)[0])
    finally:
        env.close()
