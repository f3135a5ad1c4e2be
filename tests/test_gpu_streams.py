"""The stream promise of include/squigly_hip.h -- "the call only enqueues work on hip_stream" -- held on a stream where it can fail:
a non-blocking side stream (torch.cuda.Stream()) with work pending in front of the call.  On the null stream, where every other GPU
test runs, a launch on the wrong stream, a missing event edge to the scene's internal stream, an unordered fill of the generator-word
table and a host buffer read after the call returned all give the bit-exact frame.

The rig (gate, poison in, poison out, consumer, host, control), what it sees and where the expected values come from are described in
tests/stream_harness.py, which holds the rig, the jobs and the forms; the tests of the depth and sky modules drive it too."""
import ctypes as C
import os
import time

import numpy as np
import pytest

import render_options as RO
from bitcmp import bits
from scenes import ROTATED
from stream_harness import (ADAPTIVE_EPS, ADAPTIVE_TOL, FORMS, FRAMES, GATE_MARGIN, GROWN, HIP_STREAM_NON_BLOCKING, MAX_GATE_MS, N_VIEWS,
                            PARAMS, THIRD, Env, Gated, assert_results, check_outside, drive, expected_of, gate_ms_for, golden,
                            same_result as same)
from stream_harness import (job_adaptive_update, job_camera_rays, job_cast_frames, job_frames, job_intersect, job_lights,  # noqa: F401
                            job_masked, job_range, job_raycast, job_raytrace, job_views)     # (looked up by name: "job_" + job)

pytestmark = pytest.mark.gpu
DEFAULTS = RO.CAST


@pytest.fixture(scope="module")
def env(sqt, O, product_scene, oracle_scene):
    import torch
    assert sqt.device_count() >= 1, "no HIP device: the product has no CPU fallback"
    e = Env(sqt, torch, O, product_scene[0], oracle_scene[0])
    yield e
    e.close()


# ---- 1. every entry point, every schedule that owns a stream edge ----------------------------------------------------
@pytest.mark.parametrize("entry_point, job, form", PARAMS, ids=[f"{ep}-{job}-{form}" for ep, job, form in PARAMS])
def test_entry_point_on_a_gated_side_stream(env, entry_point, job, form):
    ds = env.scene_for(form)
    try:
        env.set_options(ds, **FORMS[form])
        built = globals()["job_" + job](env, ds)
        want = drive(env, built, env.side, f"{job}-{form}")
        assert entry_point in env.L.names, (entry_point, env.L.names)
        check_outside(env, job, want)
        if job == "adaptive_update":                            # the rule, restated in numpy on the same moments
            b = {name: value for name, _, value in built[0] if isinstance(value, np.ndarray)}
            ref = env.sqt.rule_reference(b["sums"], b["sums2"], b["counts"], b["mask"], ADAPTIVE_TOL, ADAPTIVE_EPS)
            assert np.array_equal(want["mask"], ref)
    finally:
        env.torch.cuda.synchronize()
        if job == "lights":
            ds.set_lights(None)
            env.torch.cuda.synchronize()
        env.set_options(ds)


# ---- 2. non-vacuity: the gate holds back its own stream only, and that stream is non-blocking ------------------------
def gate_holds_only_its_stream(env, side):
    """The control: inputs gated on `side`, the query issued on the null stream.  True when the query read the poison (the
    result differs from the expected one), i.e. when a gate on `side` does not hold back other streams."""
    torch = env.torch
    env.set_options(env.ds)
    job = job_intersect(env, env.ds)
    want, gate_ms = expected_of(env, job, "control")
    g = Gated(env, job, side, "control")
    torch.cuda.synchronize()
    t_gate = time.perf_counter()
    env.gate(side, gate_ms)
    with torch.cuda.stream(side):
        for name in g.src:
            g.B[name].copy_(g.src[name])
    g.steps[0](g.B, None, lambda *host, waits=None: None)         # the wrong caller: the null stream
    pending = side.query() is False and (time.perf_counter() - t_gate) * 1e3 < GATE_MARGIN * gate_ms
    torch.cuda.synchronize()
    tri = g.B["tri"].cpu().numpy()
    differs = not np.array_equal(tri, want["tri"])
    print(f"[streams] control: gate still closed after the call: {pending}; misses {int((tri < 0).sum())} of {tri.size} "
          f"(expected {int((want['tri'] < 0).sum())}); result differs: {differs}")
    return pending and differs


def test_control_a_gate_on_the_side_stream_does_not_hold_back_the_null_stream(env):
    ok = gate_holds_only_its_stream(env, env.side)
    if not ok:                                                  # two streams can share a hardware queue: try another stream object
        for other in env.streams[1:]:
            if gate_holds_only_its_stream(env, other):
                print("[streams] control: the first side stream is blind on this machine, another stream object is not")
                break
    assert ok, "a gate on the module's side stream holds back the null stream too: the rig cannot see work on a wrong stream"
    assert gate_holds_only_its_stream(env, env.side2), "the second side stream (two scenes, two streams) is blind"


def hip_runtime():
    """The HIP runtime this process has already loaded (the one the streams were made by), through ctypes."""
    for line in open("/proc/self/maps"):
        path = line.split()[-1]
        if "libamdhip64.so" in os.path.basename(path):
            return C.CDLL(path)
    raise AssertionError("no libamdhip64.so is loaded into this process")


def test_the_side_streams_are_non_blocking(env):
    hip = hip_runtime()
    hip.hipStreamGetFlags.argtypes = [C.c_void_p, C.POINTER(C.c_uint)]
    hip.hipStreamGetFlags.restype = C.c_int
    for s in env.streams:
        flags = C.c_uint(0xFFFFFFFF)
        assert hip.hipStreamGetFlags(C.c_void_p(s.cuda_stream), C.byref(flags)) == 0
        assert flags.value & HIP_STREAM_NON_BLOCKING, flags.value
        assert s.cuda_stream != 0
    assert env.torch.cuda.current_stream().cuda_stream == 0       # what every other GPU test runs on: the null stream


# ---- 3. the table of generator words is filled on the caller's stream ------------------------------------------------
def test_generator_word_table_is_filled_and_grown_on_the_side_stream(env):
    torch, sqt = env.torch, env.sqt
    env.set_options(env.ds)
    torch.cuda.synchronize()
    sqt.lib().sq_release_cached_memory()                         # no kept table: the fresh scene has to fill its own
    fresh = sqt.DeviceScene(env.bih, 0)
    try:
        assert fresh.rng_table()[0] == 0
        covers = []
        # The scene's first frame allocates its workspace and its table but frees nothing: it is held to the host check like a warm
        # call, so its fill of the table and all its launches are enqueued with the gate closed.  The larger frame outgrows the table
        # and frees the old block, which waits for the device (include/squigly_hip.h): that call alone is exempt from the host check.
        # By the time its launches are enqueued the gate has opened, so for it the rig shows only that the frame and the new table's
        # contents are right, not that nothing ran early.
        for frames, why in (((FRAMES[0],), None),
                            ((GROWN,), "a larger frame grows the table: the old block is freed, which waits for the device")):
            want, gate_ms = expected_of(env, job_frames(env, env.ds, frames=frames), f"table {frames[0][:3]}")
            bufs, steps = job_frames(env, fresh, frames=frames)
            cold = [lambda B, sp, called, step=steps[0]: step(B, sp, lambda *host, waits=None: called(*host, waits=why))]
            g = Gated(env, (bufs, cold), env.side, f"table {frames[0][:3]}")
            torch.cuda.synchronize()
            g.arm(gate_ms)
            g.run()
            g.finish()
            torch.cuda.synchronize()
            assert_results(g.results(), want, g.label)
            cover, words = fresh.rng_table(0, 64)
            covers.append(cover)
            assert cover > 0 and np.array_equal(words, sqt.debug_eval("tfgen3", np.arange(64)))
            tail = fresh.rng_table(cover - 64, 64)[1]
            assert np.array_equal(tail, sqt.debug_eval("tfgen3", np.arange(cover - 64, cover)))
        assert covers[1] > covers[0], covers                    # the table grew, and was filled again on the side stream
        # warm now: the same frame again only enqueues
        drive(env, job_frames(env, fresh, frames=(GROWN,)), env.side, "table warm")
    finally:
        torch.cuda.synchronize()
        fresh.close()


# ---- 4. two scenes, two streams ----------------------------------------------------------------------------------------
def test_two_scenes_on_two_streams_share_nothing(env):
    torch, sqt = env.torch, env.sqt
    a, b = sqt.DeviceScene(env.bih, 0), sqt.DeviceScene(env.bih, 0)
    try:
        for ds in (a, b):
            for k, v in DEFAULTS.items():
                ds.set_option(k, v)
        job_a = job_frames(env, a, tag="a_")                     # data/camera, both shapes
        fb, ib = job_frames(env, b, cam_text=ROTATED, tag="b_"), job_intersect(env, b, tag="b_")
        job_b = (ib[0] + fb[0], ib[1] + fb[1])                   # an intersect, then the frames of another camera
        want_a, gate_a = expected_of(env, job_a, "two scenes, a")
        want_b, gate_b = expected_of(env, job_b, "two scenes, b")
        assert not same(want_a["a_avg0"], want_b["b_avg0"])       # different cameras
        gate_ms = min(MAX_GATE_MS, gate_a + gate_b)
        ga, gb = Gated(env, job_a, env.side, "two scenes, a"), Gated(env, job_b, env.side2, "two scenes, b")
        torch.cuda.synchronize()
        ga.arm(gate_ms)
        gb.arm(gate_ms)
        ga.run((0,))                                            # a renders ...
        gb.run((0,))                                            # ... while b intersects
        gb.run((1,))
        ga.run((1,))
        gb.run((2,))
        ga.finish()
        gb.finish()
        torch.cuda.synchronize()
        assert_results(ga.results(), want_a, ga.label)
        assert_results(gb.results(), want_b, gb.label)
    finally:
        torch.cuda.synchronize()
        a.close()
        b.close()


# ---- 5. the stream= argument of the Python wrappers: outputs are allocated under the call's stream ------------------
def _wrapper_calls(env):
    """name -> (shape of the wrapper's first allocation, call(stream) -> the tensors to compare, golden file of the first or None)."""
    torch, ds, dev = env.torch, env.ds, env.dev
    w, h, spp, _ = FRAMES[0]
    vw, vh, vspp = 40, 72, 3
    mk = lambda shape, dt, v: torch.full(shape, v, dtype=dt, device=dev)     # noqa: E731
    given = {"sums": mk((w, h, 3), torch.float32, 7.25), "sums2": mk((w, h, 3), torch.float32, 5.5), "counts": mk((w, h), torch.int32, 0),
             "mask": mk((w, h), torch.uint8, 1)}
    cams = lambda: [env.new_cam(), env.new_cam(ROTATED), env.new_cam(THIRD)]  # noqa: E731
    return {
        "render_rows": ((w, h, 3), lambda st: ds.render_rows(env.new_cam(), spp, w, h, stream=st), "scene_64x64_4spp_avg.npy"),
        "render_rows_range": ((w, h, 3), lambda st: ds.render_rows_range(env.new_cam(), spp, w, h, 0, spp, given["sums"], stream=st),
                              "scene_64x64_4spp_avg.npy"),
        "render_rows_masked": ((w, h, 3), lambda st: ds.render_rows_masked(env.new_cam(), spp, w, h, 0, spp, given["sums"], mask=given["mask"],
                                                                           sums2=given["sums2"], counts=given["counts"], stream=st),
                               "scene_64x64_4spp_avg.npy"),
        "render_views": ((N_VIEWS, vw, vh, 3), lambda st: ds.render_views(cams(), vspp, vw, vh, stream=st), "scene_40x72_3spp_avg.npy"),
        "camera_rays": ((vw, vh, 3), lambda st: ds.camera_rays(env.new_cam(ROTATED), vw, vh, stream=st), None),
    }


@pytest.mark.parametrize("wrapper", ("render_rows", "render_rows_range", "render_rows_masked", "render_views", "camera_rays"))
def test_wrapper_allocates_its_outputs_under_the_stream_it_is_given(env, wrapper):
    """A block that the current stream has just released, with a fill of it still pending there, must not become the output of a
    call on another stream: the pending fill would overwrite the frame.  Whatever the allocator does, the returned tensors hold
    the golden values."""
    torch = env.torch
    env.set_options(env.ds)
    shape, call, gold = _wrapper_calls(env)[wrapper]
    want = [t.cpu().numpy() for t in call(None)]                 # the null stream; .cpu() waits
    t0 = time.perf_counter()
    call(None)
    gate_ms = gate_ms_for((time.perf_counter() - t0) * 1e3)
    torch.cuda.synchronize()
    side, current = env.side, torch.cuda.current_stream()
    torch.cuda.empty_cache()
    t_gate = time.perf_counter()
    env.gate(current, gate_ms)
    t = torch.empty(shape, dtype=torch.float32, device=env.dev)
    t.fill_(777.0)
    ptr = t.data_ptr()
    del t
    out = call(side)                                            # `side` is idle: the call runs at once, the fill long after it
    assert current.query() is False and (time.perf_counter() - t_gate) * 1e3 < GATE_MARGIN * gate_ms, \
        "the fill was no longer pending when the call returned: the call blocked the host, or the gate was too short"
    reused = [o.data_ptr() == ptr for o in out]
    side.synchronize()
    torch.cuda.synchronize()
    got = [o.cpu().numpy() for o in out]
    print(f"[streams] {wrapper}(stream=side): released block handed out again: {reused}; values of 777.0 in the outputs: "
          f"{[int((g == 777.0).sum()) for g in got]}")
    for g, e in zip(got, want):
        assert same(g, e), (wrapper, int((bits(g) != bits(e)).sum()), g.reshape(-1)[:6])
    if gold is not None:
        first = got[0][0] if wrapper == "render_views" else got[0]
        assert same(first, golden(gold).reshape(first.shape))
