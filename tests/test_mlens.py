"""Masked lens frames without a GPU: the surface of libsquigly_mlens.so -- the header, the exports, the ids, every refusal that needs
no device -- the Python layer's refusals, render_adaptive(lens=None) as the code path it was, the numpy restatement
(tests/mlens_restatement.py) on hand-made inputs, and the populations of its adaptive driver, which keep the GPU tests' per-pixel
pins from being vacuous."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import lens_restatement as LR
import library_surface as LS
import mlens_restatement as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NO_DEVICE = 1 << 20         # a device number no machine has: a call the checks let through by mistake fails there, before any launch
W, H, P = MR.W, MR.H, MR.P


@pytest.fixture(scope="module")
def mlens(sqt):
    mod = importlib.import_module("squigly-trace_amd.mlens")
    mod.lib()
    return mod


@pytest.fixture(scope="module")
def lens(sqt):
    mod = importlib.import_module("squigly-trace_amd.lens")
    mod.lib()
    return mod


# ---- the library's surface ----
def header_text():
    return open(os.path.join(ROOT, "include", "squigly_mlens.h")).read()


def test_header_carries_the_contract_and_the_pins():
    text = header_text()
    for line in ("LIVE p = (d_mask == NULL || d_mask[p] != 0) && (r_begin == 0 || d_count == NULL || d_count[p] == r_begin)",
                 "list   = the live pixels in ascending order, L of them",
                 "ray slot (r - r_begin) * L + j",
                 "s_r  = sq_raytrace_rays_device's d_sum for (o, d, seed = base), k in [0, n)",
                 "sum  = s_0 when r_begin == 0, else what d_sum[p] holds ;  sum = sum + s_r in the order of r ;  sum2 likewise of s_r * s_r",
                 "count = r_end",
                 "avg  = (1 / (float) (r_end * n)) *^ sum ;  rgb = rgbFloatToPixelRGB avg",
                 "a pixel that is not listed is written in none of d_sum, d_sum2, d_count, d_avg, d_rgb",
                 "1. With the full list (NULL mask, r_begin = 0), sum and sum2 are sq_lens_render_device's bits for any lens",
                 "2. With jitter = aperture = 0 and R = S, all five buffers are sq_render_rows_device_masked's bits",
                 "3. Consecutive ranges give the bits of one call, and the result does not depend on the batching",
                 "An entry outside [0, P) gets o = d = +0 and seed 0", "An entry outside [0, P) is skipped",
                 "PRECONDITION: the list is strictly ascending", "A duplicate entry is a caller error"):
        assert line in text, line
    for word in ("INDEX WIDTHS", "2^31 - 1", "HOST WAIT", "44 bytes", "SUB-RAYS", "Out of scope", "sq_lens_plan(L, r_begin, r_end, work_bytes)"):
        assert word in text, word
    # the lens header points here, and kept what tests/test_lens.py looks for
    lens_text = open(os.path.join(ROOT, "include", "squigly_lens.h")).read()
    assert "Out of scope" in lens_text and "squigly_mlens.h" in lens_text


def test_header_functions_are_exported(mlens):
    declared = LS.check_exports(mlens, "squigly_mlens.h", "sq_mlens_")       # (no planner export, nothing of the other libraries')
    assert declared == {"sq_mlens_last_error", "sq_mlens_build_id", "sq_mlens_live_device", "sq_mlens_rays_device", "sq_mlens_fold_device",
                        "sq_mlens_render_device"}


def test_the_other_libraries_did_not_gain_it(sqt, lens, mlens):
    for h in ("squigly_hip.h", "squigly_host.h", "squigly_denoise.h"):
        assert "sq_mlens" not in open(os.path.join(ROOT, "include", h)).read(), h
    assert not [s for s in sqt.EXPORTED_SYMBOLS + lens.EXPORTED_SYMBOLS if "mlens" in s]
    for path in (sqt.LIB_PATH, lens.LIB_PATH):
        assert "sq_mlens" not in subprocess.check_output(["nm", "-D", "--defined-only", path]).decode(), path
    b = LS.build_module()
    mine = {"sq_mlens.hip", "../../include/squigly_mlens.h"}
    assert not mine & set(LS.files(b, "main", "denoise", "lens"))
    assert mine | {"sq_lens_plan.h", "sq_lens_ray.h", "../../include/squigly_lens.h"} <= set(LS.files(b, "mlens"))
    assert "sq_lens_ray.h" in b.LIBS["lens"]["headers"]          # the contract is written once, and both ids follow it
    assert "sq_lens_frame.h" in b.LIBS["lens"]["headers"] and "sq_lens_frame.h" in b.LIBS["mlens"]["headers"]      # ... and so are the kernels and the batch loop
    assert "sq_lens_frame.h" not in LS.files(b, "main", "denoise")
    assert b.LIBS["mlens"]["link"] == b.LIBS["lens"]["link"]
    assert b.LIBS["mlens"]["salt"] not in (b.LIBS["lens"]["salt"], b.LIBS["main"]["salt"], b.LIBS["denoise"]["salt"])
    LS.check_client(mlens.LIB_PATH, True, never=("libsquigly_lens",))


def test_ids_are_separate(lens, mlens, sqt, tmp_path):
    b = LS.build_module()
    assert lens.build_id() == b.lib_source_id(b.LIBS["lens"])
    own, shared = {"mlens"}, {"lens", "mlens", "shutter"}        # (the shutter library reads the lens libraries' shared text too)
    LS.check_ids(b, "mlens", mlens, sqt, tmp_path, [("sq_mlens.hip", own), ("../../include/squigly_mlens.h", own), ("sq_lens_ray.h", shared),
                                                    ("sq_lens_plan.h", shared), ("sq_lens_frame.h", shared)])


# ---- refusals: nothing here reaches a device, the buffer pointers are numbers that are never followed ----
BUF = {name: 0x10000000 + i * 0x1000000 for i, name in
       enumerate(("org", "dir", "seed", "part", "sum", "sum2", "avg", "rgb", "work", "index", "count", "mask", "n_live"))}
SCENE = 0x7000000
FAR = {name: (i + 1) << 40 for i, name in enumerate(BUF)}
nan, inf = float("nan"), float("inf")


def frame_call(sqt, mlens, lens, which, cam=True, lens_values=(1.0, 0.0, 1.0), null_lens=False, S=8, R=4, r=(0, 4), w=W, h=H, shard=None,
               L=100, work_bytes=None, device=NO_DEVICE, **ptr):
    lib = mlens.lib()
    a = {**BUF, **ptr}
    c = sqt.load_camera(os.path.join(ROOT, "data", "camera"))
    ln = lens.Lens.__new__(lens.Lens)                       # unchecked values: the library's own checks are what is under test
    C.Structure.__init__(ln, *lens_values)
    sh = sqt.Shard(*(shard or (w if w > 0 else 1, 0, 1)))
    head = [C.byref(c) if cam else None, None if null_lens else C.byref(ln), S, R, r[0], r[1], w, h, sh, a["index"], L]
    if which == "rays":
        rc = lib.sq_mlens_rays_device(device, *head, a["org"], a["dir"], a["seed"], None)
    else:
        wb = lens.work_bytes(max(L, 1), 1) if work_bytes is None else work_bytes
        rc = lib.sq_mlens_render_device(a.get("scene", SCENE), *head, a["work"], wb, a["sum"], a["sum2"], a["count"], a["avg"], a["rgb"], None)
    return rc, lib.sq_mlens_last_error().decode()


FRAME_REFUSALS = [
    (dict(cam=False), "null argument"), (dict(null_lens=True), "null argument"),
    (dict(S=0), "at least 1"), (dict(R=0), "at least 1"), (dict(S=-8), "at least 1"), (dict(S=8, R=3), "must divide"),
    (dict(S=4, R=8, r=(0, 8)), "must divide"),
    (dict(r=(-1, 4)), "bad sub-ray range"), (dict(r=(2, 2)), "bad sub-ray range"), (dict(r=(3, 2)), "bad sub-ray range"),
    (dict(r=(0, 5)), "bad sub-ray range"),
    (dict(lens_values=(-0.1, 0.0, 1.0)), "jitter"), (dict(lens_values=(1.5, 0.0, 1.0)), "jitter"), (dict(lens_values=(nan, 0.0, 1.0)), "jitter"),
    (dict(lens_values=(1.0, -0.5, 1.0)), "aperture"), (dict(lens_values=(1.0, inf, 1.0)), "aperture"),
    (dict(lens_values=(1.0, 0.1, 0.0)), "focus"), (dict(lens_values=(1.0, 0.1, nan)), "focus"), (dict(lens_values=(1.0, 0.1, inf)), "focus"),
    (dict(w=0), "at least 1"), (dict(h=0), "at least 1"),
    (dict(shard=(2, 3, 3)), "bad shard"), (dict(shard=(0, 0, 1)), "bad shard"),
    (dict(w=46341, h=46341, work_bytes=1 << 50), r"exceed 2\^31 - 1 pixels"),
    (dict(index=None), "d_index is required"), (dict(L=-1), "the list must hold"), (dict(L=P + 1), "the list must hold"),
]
RAYS_REFUSALS = FRAME_REFUSALS + [
    (dict(org=None), "null argument"), (dict(dir=None), "null argument"), (dict(seed=None), "null argument"),
    (dict(w=1024, h=1024, S=4096, R=4096, r=(0, 2048), L=2 ** 20, **FAR), r"exceed 2\^31 - 1 ray slots"),       # 2^20 listed pixels x 2^11 sub-rays
    (dict(dir=BUF["org"] + 12 * 100 * 4 - 4), "d_org and d_dir overlap"), (dict(seed=BUF["org"]), "d_org and d_seed overlap"),
    (dict(index=BUF["org"] + 8), "d_index and d_org overlap"), (dict(index=BUF["seed"] - 4), "d_index and d_seed overlap"),
]
RENDER_REFUSALS = FRAME_REFUSALS + [
    (dict(scene=None), "null argument"), (dict(work=None), "null argument"), (dict(sum=None), "null argument"),
    (dict(work_bytes=4399), "too small"), (dict(work_bytes=0), "too small"),                    # 100 pixels: 4400 bytes a sub-ray
    (dict(work=BUF["work"] + 8), "16-byte aligned"),
    (dict(sum2=BUF["sum"] + 12), "d_sum and d_sum2 overlap"), (dict(avg=BUF["sum"]), "d_sum and d_avg overlap"),
    (dict(rgb=BUF["avg"] + 12 * P - 1), "d_avg and d_rgb overlap"), (dict(count=BUF["sum2"] + 12 * P - 4), "d_sum2 and d_count overlap"),
    (dict(index=BUF["count"] + 4 * P - 4), "d_index and d_count overlap"), (dict(index=BUF["sum"]), "d_index and d_sum overlap"),
    (dict(work=BUF["sum"] - 16), "d_sum and d_work overlap"), (dict(index=BUF["work"] + 4400 - 4), "d_index and d_work overlap"),
]


@pytest.mark.parametrize("kw, message", RAYS_REFUSALS, ids=[f"{i:02d}-{m[:12]}" for i, (_, m) in enumerate(RAYS_REFUSALS)])
def test_rays_refusals_need_no_gpu(sqt, mlens, lens, kw, message):
    rc, err = frame_call(sqt, mlens, lens, "rays", **kw)
    assert rc != 0 and re.search(message, err), err


@pytest.mark.parametrize("kw, message", RENDER_REFUSALS, ids=[f"{i:02d}-{m[:12]}" for i, (_, m) in enumerate(RENDER_REFUSALS)])
def test_render_refusals_need_no_gpu(sqt, mlens, lens, kw, message):
    rc, err = frame_call(sqt, mlens, lens, "render", **kw)
    assert rc != 0 and re.search(message, err), err


def test_live_and_fold_refusals(mlens):
    lib, B = mlens.lib(), BUF
    err = lambda: lib.sq_mlens_last_error().decode()  # noqa: E731
    ok = dict(P=P, r=0, mask=B["mask"], count=B["count"], index=B["index"], n_live=B["n_live"])
    for kw, message in ((dict(index=None), "null argument"), (dict(n_live=None), "null argument"), (dict(P=0), "at least 1"), (dict(P=-3), "at least 1"),
                        (dict(P=2 ** 31), r"exceed 2\^31 - 1 pixels"), (dict(r=-1), "r_begin must be at least 0"),
                        (dict(index=B["mask"]), "d_mask and d_index overlap"), (dict(index=B["count"] + 4 * P - 4), "d_count and d_index overlap"),
                        (dict(n_live=B["index"] + 8), "d_index and d_n_live overlap"), (dict(n_live=B["count"]), "d_count and d_n_live overlap")):
        a = {**ok, **kw}
        assert lib.sq_mlens_live_device(NO_DEVICE, a["P"], a["r"], a["mask"], a["count"], a["index"], a["n_live"], None) != 0
        assert re.search(message, err()), (kw, err())
    for kw in (dict(), dict(mask=None), dict(count=None), dict(mask=None, count=None, r=5), dict(P=2 ** 31 - 1, mask=FAR["mask"], count=FAR["count"], index=FAR["index"])):
        a = {**ok, **kw}
        assert lib.sq_mlens_live_device(NO_DEVICE, a["P"], a["r"], a["mask"], a["count"], a["index"], a["n_live"], None) != 0
        assert "hipSetDevice" in err(), (kw, err())

    ok = dict(P=P, S=8, R=4, r=(0, 4), index=B["index"], L=100, part=B["part"], sum=B["sum"], sum2=B["sum2"], count=B["count"], avg=B["avg"], rgb=B["rgb"])

    def fold(a):
        return lib.sq_mlens_fold_device(NO_DEVICE, a["P"], a["S"], a["R"], a["r"][0], a["r"][1], a["index"], a["L"], a["part"], a["sum"], a["sum2"],
                                        a["count"], a["avg"], a["rgb"], None)
    for kw, message in ((dict(part=None), "null argument"), (dict(sum=None), "null argument"), (dict(index=None), "d_index is required"),
                        (dict(P=0), "at least 1"), (dict(S=0), "at least 1"), (dict(R=0), "at least 1"), (dict(R=3), "must divide"),
                        (dict(r=(-1, 4)), "bad sub-ray range"), (dict(r=(4, 4)), "bad sub-ray range"), (dict(r=(0, 5)), "bad sub-ray range"),
                        (dict(P=2 ** 31), r"exceed 2\^31 - 1 pixels"), (dict(L=-1), "the list must hold"), (dict(L=P + 1), "the list must hold"),
                        (dict(P=2 ** 20, L=2 ** 20, S=4096, R=4096, r=(0, 2048), **{k: FAR[k] for k in ("index", "part", "sum", "sum2", "count", "avg", "rgb")}),
                         r"exceed 2\^31 - 1 ray slots"),
                        (dict(sum=B["part"] + 12 * 100 * 4 - 4), "d_part and d_sum overlap"), (dict(sum2=B["sum"]), "d_sum and d_sum2 overlap"),
                        (dict(count=B["sum2"] + 12), "d_sum2 and d_count overlap"), (dict(avg=B["count"]), "d_count and d_avg overlap"),
                        (dict(rgb=B["part"]), "d_part and d_rgb overlap"), (dict(index=B["part"] + 12 * 400 - 4), "d_index and d_part overlap")):
        assert fold({**ok, **kw}) != 0 and re.search(message, err()), (kw, err())
    for kw in (dict(), dict(sum2=None, count=None, avg=None, rgb=None), dict(r=(3, 4)), dict(L=P)):
        assert fold({**ok, **kw}) != 0 and "hipSetDevice" in err(), (kw, err())
    assert fold({**ok, "L": 0}) == 0                                     # an empty list is no error and touches nothing


def test_what_is_allowed_gets_past_the_checks(sqt, mlens, lens):
    for kw in (dict(), dict(lens_values=(0.0, 0.0, -1.0)), dict(lens_values=(1.0, 0.25, 3.0)), dict(L=P), dict(L=1), dict(r=(3, 4)),
               dict(w=1024, h=1024, S=4096, R=4096, r=(0, 2047), L=2 ** 20, **FAR)):
        rc, err = frame_call(sqt, mlens, lens, "rays", **kw)
        assert rc != 0 and "hipSetDevice" in err, err
    for kw in (dict(), dict(sum2=None, count=None, avg=None, rgb=None), dict(work_bytes=1 << 20), dict(r=(1, 3)), dict(L=P, work_bytes=44 * P)):
        rc, err = frame_call(sqt, mlens, lens, "render", **kw)
        assert rc != 0 and "hipPointerGetAttributes" in err, err
    for which in ("rays", "render"):
        assert frame_call(sqt, mlens, lens, which, w=4, shard=(2, 2, 3))[0] == 0            # an empty shard
        assert frame_call(sqt, mlens, lens, which, L=0)[0] == 0                            # an empty list


# ---- the Python layer ----
def test_python_refusals(sqt, mlens):
    E = sqt.SquiglyError
    ds = object.__new__(sqt.DeviceScene)        # a scene that was never uploaded: whatever gets past its refusal would fail in some other way
    ds.device, ds._h = 0, None
    cam = sqt.load_camera(os.path.join(ROOT, "data", "camera"))
    ln = sqt.Lens()
    rm = lambda **kw: ds.render_lens_masked(cam, kw.pop("lens", ln), kw.pop("S", 8), kw.pop("R", 4), W, H, kw.pop("r0", 0), kw.pop("r1", 4),  # noqa: E731
                                            kw.pop("sums", None), None, kw.pop("n_live", 1), **kw)
    for call, message in ((lambda: rm(R=3), "must divide"), (lambda: rm(lens=None), "lens must be a Lens"), (lambda: rm(r1=5), "bad sub-ray range"),
                          (lambda: rm(r0=2, r1=2), "bad sub-ray range"), (lambda: rm(work_mb=0), "work_mb"), (lambda: rm(shard=(2, 3, 3)), "bad shard"),
                          (lambda: rm(n_live=-1), "n_live must be between"), (lambda: rm(n_live=P + 1), "n_live must be between"),
                          (lambda: rm(n_live=1.0), "n_live must be an integer"), (lambda: rm(), "needs a sums tensor"),
                          (lambda: ds.live_pixels(None, None, 0), "needs a mask or the counts"), (lambda: ds.live_pixels(np.ones((W, H), np.uint8), None, 0), "CUDA tensors"),
                          (lambda: ds.live_pixels(None, None, -1), "r_begin must be at least 0"), (lambda: ds.live_pixels(None, None, 1.5), "r_begin must be an integer")):
        with pytest.raises(E, match=message):
            call()
    ok = dict(samples=8, subrays=4, w=8, h=8, tol=0.5)
    for kw in (dict(tol=-0.1), dict(tol=nan), dict(eps=-1.0), dict(first=0), dict(step=0), dict(done=-1), dict(done=5), dict(done=2), dict(rule=3)):
        a = {**ok, **kw}
        with pytest.raises(ValueError):
            sqt.AdaptiveLens(None, None, ln, a.pop("samples"), a.pop("subrays"), a.pop("w"), a.pop("h"), a.pop("tol"), **a)
    for args, message in (((None, 8, 4), "lens must be a Lens"), ((ln, 8, 3), "must divide"), ((ln, 0, 1), "at least 1")):
        with pytest.raises(E, match=message):
            sqt.AdaptiveLens(None, None, args[0], args[1], args[2], 8, 8, 0.5)
    with pytest.raises(E, match="bad shard"):
        sqt.AdaptiveLens(None, None, ln, 8, 4, 8, 8, 0.5, shard=(2, 3, 3))
    # render_adaptive with a lens: refused before a scene is uploaded
    for kw, exc in ((dict(lens=ln, subrays=4, first=3), ValueError), (dict(lens=ln, subrays=4, step=5), ValueError), (dict(lens=ln, cast=True), ValueError),
                    (dict(subrays=4), ValueError), (dict(lens=ln, subrays=3), E), (dict(lens=(1, 0, 1)), E), (dict(lens=ln, subrays=4, depth=9), E),
                    (dict(lens=ln, subrays=4, first=0), ValueError), (dict(lens=ln, subrays=4, denoise=-1.0), ValueError)):
        with pytest.raises(exc):
            next(sqt.render_adaptive(None, cam, 8, (W, H), 0.5, **{"first": 2, "step": 2, **kw}))
    assert sqt.AdaptiveLens is importlib.import_module("squigly-trace_amd.device").AdaptiveLens


def test_render_adaptive_without_a_lens_is_the_code_path_it_was(sqt, monkeypatch):
    """lens=None: the same constructor call, the same steps and the same tuples as before the lens existed -- recorded on a stand-in
    for Adaptive -- and AdaptiveLens is never touched."""
    dev = importlib.import_module("squigly-trace_amd.device")
    render = importlib.import_module("squigly-trace_amd.render")
    calls = []

    class Tensor:
        def __init__(self, v):
            self.v = v

        def cpu(self):
            return self

        def numpy(self):
            return self.v

    class FakeAdaptive:
        def __init__(self, *args, **kw):
            calls.append(("init", args[2:], kw))
            self.done, self.live, self.samples_spent, self.counts, self.left = 0, 7, 0, Tensor("counts"), 2

        finished = property(lambda self: self.left == 0)

        def step(self):
            calls.append(("step",))
            self.left -= 1
            self.done += 8
            return Tensor("avg"), Tensor("rgb")

    class Scene:
        def __enter__(self):
            return "ds"

        def __exit__(self, *a):
            calls.append(("closed",))

    def no_lens(*a, **kw):
        raise AssertionError("AdaptiveLens on the path without a lens")
    monkeypatch.setattr(dev, "Adaptive", FakeAdaptive)
    monkeypatch.setattr(dev, "AdaptiveLens", no_lens)
    monkeypatch.setattr(render, "_resident", lambda *a: calls.append(("resident", a)) or Scene())
    out = list(sqt.render_adaptive("bih", "cam", 16, (W, H), 0.5, eps=0.25, first=4, step=2, cast=True, device=3, rule=None, lights="L", depth=5, sky="S"))
    assert out == [(8, 7, 0, "rgb", "counts"), (16, 7, 0, "rgb", "counts")]
    assert calls == [("resident", ("bih", 3, "L", 5, "S")),
                     ("init", (16, W, H, 0.5), dict(eps=0.25, first=4, step=2, cast=True, rule=None)), ("step",), ("step",), ("closed",)]


# ---- the restatement ----
def test_live_rule_and_list():
    mask = np.array([1, 0, 2, 1, 0, 255, 1], np.uint8)
    counts = np.array([4, 4, 3, 4, 4, 4, 0], np.int32)
    assert MR.live_list(mask, counts, 0).tolist() == [0, 2, 3, 5, 6]            # r_begin = 0: the counts take no part
    assert MR.live_list(mask, counts, 4).tolist() == [0, 3, 5]                   # the gap guard
    assert MR.live_list(None, counts, 4).tolist() == [0, 1, 3, 4, 5]
    assert MR.live_list(mask, None, 4).tolist() == [0, 2, 3, 5, 6]
    assert MR.live_list(None, None, 9, pixels=3).tolist() == [0, 1, 2]
    assert MR.live_list(np.zeros(5, np.uint8), None, 0).dtype == np.int32 and len(MR.live_list(np.zeros(5, np.uint8), None, 0)) == 0


def test_indexed_fold_equals_the_lens_fold_on_the_listed_pixels():
    rng = np.random.default_rng(5)
    parts = (rng.standard_normal((6, 9, 3)) * 10.0 ** rng.integers(-3, 4, (6, 9, 3))).astype(f32)
    parts[0, 2] = -0.0
    index = np.array([1, 4, 5, 8], np.int32)
    n, S = 2, 12
    fresh = lambda: {"sum": np.full((9, 3), 7.25, f32), "sum2": np.full((9, 3), 5.5, f32), "count": np.full(9, 77, np.int32),  # noqa: E731
                     "avg": np.full((9, 3), -3.5, f32), "rgb": np.full((9, 3), 123, np.uint8)}
    st = MR.indexed_fold(parts[:, index], index, n, 0, 6, fresh())
    s, q, avg = LR.fold(parts, S)
    for k, want in (("sum", s), ("sum2", q), ("avg", avg)):                         # r_end = R: the divisor is S
        assert np.array_equal(st[k][index].view(np.uint32), want[index].view(np.uint32)), k
    dead = np.setdiff1d(np.arange(9), index)
    assert (st["sum"][dead] == 7.25).all() and (st["sum2"][dead] == 5.5).all() and (st["count"][dead] == 77).all()
    assert (st["avg"][dead] == -3.5).all() and (st["rgb"][dead] == 123).all() and (st["count"][index] == 6).all()
    # in ranges, with the pixel's own divisor, and entries outside [0, P) skipped
    wild = np.array([-1, 1, 4, 5, 8, 9], np.int32)
    padded = np.concatenate([np.full((6, 1, 3), 9e9, f32), parts[:, index], np.full((6, 1, 3), 9e9, f32)], axis=1)
    a = MR.indexed_fold(padded[:4], wild, n, 0, 4, fresh())
    s4, _, _ = LR.fold(parts, S, (0, 4))
    with np.errstate(all="ignore"):
        assert np.array_equal(a["avg"][index].view(np.uint32), ((f32(1) / f32(8)) * s4[index]).astype(f32).view(np.uint32))
    assert (a["count"][index] == 4).all() and (a["sum"][dead] == 7.25).all()
    b = MR.indexed_fold(padded[4:], wild, n, 4, 6, a)
    for k in ("sum", "sum2", "avg", "rgb", "count"):
        assert np.array_equal(b[k], st[k]), k


@pytest.mark.parametrize("case", list(MR.CASES))
def test_the_adaptive_drivers_populations(sqt, case):
    """Counted with the oracle when the feature was specified: (a) 326 / 27 / 9 / 22 pixels stop after 2 / 4 / 6 / 8 sub-rays, (b)
    342 / 18 / 8 / 16.  At least 5 in each class keep the GPU tests' per-pixel prefix pins from being vacuous.  (With the default
    eps = 1 nearly everything -- 374 of 384 -- stops after the first step.)"""
    lens_name, S, R, eps = MR.CASES[case]
    n = S // R
    st = MR.adaptive(MR.sub_ray_sums(lens_name, S, R), n, lambda s, q, c, m: sqt.rule_reference(s, q, c, m, MR.TOL, eps * n * n))
    classes = MR.stop_classes(st["count"], R)
    print(f"case ({case}): pixels stopping after 2 / 4 / 6 / 8 sub-rays: {classes}")
    assert sum(classes) == P and min(classes) >= 5, classes
    assert classes == {"a": [326, 27, 9, 22], "b": [342, 18, 8, 16]}[case]
    assert st["done"] == R and st["steps"] == 4
    # every pixel holds the lens fold of its own prefix and its own divisor
    parts = MR.sub_ray_sums(lens_name, S, R)
    for c in range(2, R + 1, 2):
        sel = st["count"] == c
        s, q, _ = LR.fold(parts, S, (0, c))
        assert np.array_equal(st["sum"][sel].view(np.uint32), s[sel].view(np.uint32)) and np.array_equal(st["sum2"][sel].view(np.uint32), q[sel].view(np.uint32))
        with np.errstate(all="ignore"):
            assert np.array_equal(st["avg"][sel].view(np.uint32), ((f32(1) / f32(c * n)) * s[sel]).astype(f32).view(np.uint32))
