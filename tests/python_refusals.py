"""The refusals of the Python layer, case by case: what tests/test_python_refusals.py and tests/test_gpu_python_refusals.py hold the
package to.  Belongs here: the named cases (each a callable that must raise), the environment they run in and the recorder; no test.

Two groups.  "cpu": everything the package refuses before it asks torch for a stream or the library for a device, on a scene that
was never uploaded (every call that gets past its refusal would fail in some other way).  "gpu": the tensor refusals and the frame
state refusals, which need a real scene and device: data/scene.obj at 8 x 8 pixels and 2 samples.  A CPU tensor stands in for "a
tensor on the wrong device".  Cases with two faults at once fix which one is reported.

tests/golden/python_refusals.json holds case name -> [exception type, message].  It is a transcript of the package as it was before
its rules were gathered in _plumbing.py, not of the package under test:

    python tests/python_refusals.py cpu tests/golden/python_refusals.json       (no GPU needed)
    python tests/python_refusals.py gpu tests/golden/python_refusals.json       (on an MI355X)

each run in a checkout of that earlier commit with this file copied into its tests/; a group replaces its own entries in the file
and leaves the other group's alone."""
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_FILE = os.path.join(ROOT, "tests", "golden", "python_refusals.json")
W = H = 8
SAMPLES = 2
BIG = 46341                                          # 46341 x 46341 pixels > 2^31 - 1
WAVE = (23171, 23173)                                # > 2^29 pixels, the wavefront form's limit
BAD_SHARD = (2, 3, 3)                                # shard 3 of 3


class Env:
    """What a case gets: the package and its modules, a camera, and the scene -- never uploaded ("cpu") or real ("gpu")."""

    def __init__(self, sqt, ds=None):
        import torch
        self.sqt, self.torch = sqt, torch
        self.N = importlib.import_module(sqt.__name__ + "._native")
        self.dn = importlib.import_module(sqt.__name__ + ".denoise")
        self.R = importlib.import_module(sqt.__name__ + ".render")
        self.cam = sqt.camera_from_text(open(os.path.join(ROOT, "data", "camera"), "rb").read())
        self.ds = ds if ds is not None else self.fake()
        self.dev = torch.device("cuda", 0) if ds is not None else None

    def fake(self, variant=None):
        """A DeviceScene that was never uploaded (tests/test_large.py): a call that reaches the device or an allocation fails."""
        ds = object.__new__(self.sqt.DeviceScene)
        ds.device = 0
        ds._h = None
        if variant is not None:
            ds._variant = variant
        return ds

    # device tensors of the 8 x 8 frame, and their wrong forms
    def t(self, shape, dtype="float32", device=None):
        return self.torch.zeros(shape, dtype=getattr(self.torch, dtype), device=self.dev if device is None else device)

    def wrong(self, kind, shape, dtype):
        """A tensor that is not the contiguous `dtype` tensor of `shape` on the device, in one way."""
        if kind == "shape":
            return self.t(tuple(shape)[:-1] + (shape[-1] + 1,), dtype)
        if kind == "dtype":
            return self.t(shape, "float64" if dtype != "float64" else "float32")
        if kind == "contiguity":
            t = self.t(tuple(shape)[:-1] + (2 * shape[-1],), dtype)[..., ::2]
            assert tuple(t.shape) == tuple(shape) and not t.is_contiguous()
            return t
        if kind == "device":
            return self.t(shape, dtype, device="cpu")
        raise KeyError(kind)


WRONG = ("shape", "dtype", "contiguity", "device")
RAYS = np.zeros((4, 3), np.float32)


# ---- the "cpu" group ------------------------------------------------------------------------------------------------------
def _cpu_cases():
    c = []

    def case(name, fn):
        c.append(("cpu:" + name, fn))

    # shard tuples
    for what, shard in (("row block 0", (0, 0, 1)), ("index == n", BAD_SHARD), ("negative index", (2, -1, 3)), ("no shards", (None, 0, 0))):
        case(f"frame_seeds shard {what}", lambda e, s=shard: e.sqt.frame_seeds(2, W, H, s))
        case(f"render_rows shard {what}", lambda e, s=shard: e.ds.render_rows(e.cam, SAMPLES, W, H, shard=s))
    case("frame_seeds samples 0", lambda e: e.sqt.frame_seeds(0, W, H))
    case("frame_seeds height 0", lambda e: e.sqt.frame_seeds(1, W, 0))
    case("frame_seeds samples 0 and bad shard", lambda e: e.sqt.frame_seeds(0, W, H, BAD_SHARD))
    methods = {
        "render_rows": lambda e, d, w, h, kw: d.render_rows(e.cam, SAMPLES, w, h, **kw),
        "render_rows_range": lambda e, d, w, h, kw: d.render_rows_range(e.cam, SAMPLES, w, h, 0, 1, e.torch.empty((1, 1, 3)), **kw),
        "render_rows_masked": lambda e, d, w, h, kw: d.render_rows_masked(e.cam, SAMPLES, w, h, 0, 1, e.torch.empty((1, 1, 3)), **kw),
        "render_views": lambda e, d, w, h, kw: d.render_views([e.cam, e.cam], SAMPLES, w, h, **kw),
        "Progressive": lambda e, d, w, h, kw: e.sqt.Progressive(d, e.cam, SAMPLES, w, h, **kw),
        "Adaptive": lambda e, d, w, h, kw: e.sqt.Adaptive(d, e.cam, SAMPLES, w, h, 0.1, **kw),
    }
    for name, call in methods.items():
        if name != "render_rows":
            case(f"{name} bad shard", lambda e, call=call: call(e, e.ds, W, H, {"shard": BAD_SHARD}))
        # frame sizes: 2^31 - 1 pixels for every form, 2^29 for the wavefront form (the default; cast frames and variant 1 take more)
        case(f"{name} oversized", lambda e, call=call: call(e, e.ds, BIG, BIG, {}))
        case(f"{name} oversized cast", lambda e, call=call: call(e, e.ds, BIG, BIG, {"cast": True}))
        case(f"{name} oversized variant 1", lambda e, call=call: call(e, e.fake(variant=1), BIG, BIG, {}))
        case(f"{name} oversized wavefront", lambda e, call=call: call(e, e.ds, WAVE[0], WAVE[1], {}))
        case(f"{name} bad shard and oversized", lambda e, call=call: call(e, e.ds, BIG, BIG, {"shard": BAD_SHARD}))
    case("camera_rays bad shard", lambda e: e.ds.camera_rays(e.cam, W, H, BAD_SHARD))
    case("render_views 3 views oversized", lambda e: e.ds.render_views([e.cam] * 3, 1, 2 ** 15, 2 ** 15, cast=True))
    case("render_views 3 views oversized wavefront", lambda e: e.ds.render_views([e.cam] * 3, 1, 2 ** 14, 2 ** 14))
    case("render_views no camera", lambda e: e.ds.render_views([], SAMPLES, W, H))
    case("render_views no camera and bad shard", lambda e: e.ds.render_views([], SAMPLES, W, H, shard=BAD_SHARD))
    case("render_rows_range oversized and no sums", lambda e: e.ds.render_rows_range(e.cam, 1, BIG, BIG, 0, 1, None))
    case("render_rows_masked oversized and no sums", lambda e: e.ds.render_rows_masked(e.cam, 1, BIG, BIG, 0, 1, None))

    # lights, depth, sky: the values
    for what, v in (("not a sequence", 5), ("empty", []), ("too many", [0] * 4097), ("three numbers", [(1, 2, 3)]),
                    ("power of two numbers", [((0, 0, 0), (1, 2))]), ("position of two numbers", [((0, 0), 1.0)]),
                    ("second of two", [(0, 0, 0, 1, 1, 1), "ab"]), ("a number as a light", [7])):
        case(f"lights_array {what}", lambda e, v=v: e.N.lights_array(v))
    case("set_lights empty", lambda e: e.ds.set_lights([]))
    case("set_lights bad light", lambda e: e.ds.set_lights([(1, 2, 3, 4, 5)]))
    for what, v in (("bool", True), ("float", 3.0), ("0", 0), ("9", 9), ("-1", -1), ("str", "3"), ("None", None)):
        case(f"depth_value {what}", lambda e, v=v: e.N.depth_value(v))
    case("set_depth 0", lambda e: e.ds.set_depth(0))
    case("set_depth float", lambda e: e.ds.set_depth(2.0))
    for what, a in (("str", ("abc",)), ("two numbers", ((1, 2),)), ("scalar", (1.0,)), ("down of one", ((1, 2, 3), (1,))),
                    ("down str", ((1, 2, 3), "xyz")), ("up and down bad", ((1,), (2,)))):
        case(f"sky_value {what}", lambda e, a=a: e.N.sky_value(*a))
    for what, v in (("number", 5), ("four numbers", (1, 2, 3, 4)), ("bad down", ((1, 2, 3), (1, 2))), ("bad up", ((1, 2), (1, 2, 3))),
                    ("one number", (1,)), ("str", "ab")):
        case(f"sky_pair {what}", lambda e, v=v: e.N.sky_pair(v))
    case("set_sky None with down", lambda e: e.ds.set_sky(None, (1, 1, 1)))
    case("set_sky two numbers", lambda e: e.ds.set_sky((1, 2)))
    case("set_sky bad down", lambda e: e.ds.set_sky((1, 2, 3), (1, 2)))

    # ray shapes, through the three queries
    queries = {"intersect": lambda e, o, d, **kw: e.ds.intersect(o, d, **kw), "raytrace": lambda e, o, d, **kw: e.ds.raytrace(o, d, **kw),
               "raycast": lambda e, o, d, **kw: e.ds.raycast(o, d, **kw)}
    for q, call in queries.items():
        case(f"{q} origins [4, 2]", lambda e, call=call: call(e, np.zeros((4, 2), np.float32), RAYS))
        case(f"{q} directions [4]", lambda e, call=call: call(e, RAYS, np.zeros(4, np.float32)))
        case(f"{q} origins a scalar", lambda e, call=call: call(e, 1.0, RAYS))
        case(f"{q} lists of other lengths", lambda e, call=call: call(e, [[0.0, 0.0, 0.0]], [[0.0, 0.0, 1.0], [0.0, 1.0, 0.0]]))
        case(f"{q} tensors [2, 4, 3] and [4, 2, 3]", lambda e, call=call: call(e, e.torch.zeros((2, 4, 3)), e.torch.zeros((4, 2, 3))))
        case(f"{q} both wrong", lambda e, call=call: call(e, np.zeros((4, 2)), np.zeros((5, 4))))

    # raytrace's own arguments
    rt = lambda e, **kw: e.ds.raytrace(RAYS, RAYS, **kw)                                     # noqa: E731
    case("raytrace samples 0", lambda e: rt(e, samples=0))
    case("raytrace bad rays and samples 0", lambda e: e.ds.raytrace(np.zeros((4, 2)), RAYS, samples=0))
    case("raytrace samples 0 and bad k_range", lambda e: rt(e, samples=0, k_range=(2, 2)))
    for what, k in (("empty", (2, 2)), ("negative", (-1, 2)), ("reversed", (3, 1)), ("2^31", (0, 2 ** 31))):
        case(f"raytrace k_range {what}", lambda e, k=k: rt(e, samples=4, k_range=k))
    case("raytrace seeds shape", lambda e: rt(e, seeds=np.zeros(5, np.int64)))
    case("raytrace seeds shape of a list", lambda e: rt(e, seeds=[[1, 2], [3, 4]]))
    case("raytrace seeds float64", lambda e: rt(e, seeds=np.zeros(4)))
    case("raytrace seeds float32 tensor", lambda e: rt(e, seeds=e.torch.zeros(4)))
    case("raytrace seeds bool", lambda e: rt(e, seeds=np.zeros(4, bool)))
    case("raytrace k_range and seeds shape", lambda e: rt(e, samples=4, k_range=(2, 2), seeds=np.zeros(5, np.int64)))
    case("raytrace seeds shape and dtype", lambda e: rt(e, seeds=np.zeros(5)))
    case("raytrace missing sums", lambda e: rt(e, samples=4, k_range=(1, 2)))
    case("raytrace seeds dtype and missing sums", lambda e: rt(e, samples=4, k_range=(1, 2), seeds=np.zeros(4)))
    case("raytrace sums a numpy array", lambda e: rt(e, sums=np.zeros((4, 3), np.float32)))
    case("raytrace sums a list", lambda e: rt(e, sums=[[0.0] * 3] * 4))
    case("raytrace sums on the cpu", lambda e: rt(e, sums=e.torch.zeros((4, 3))))
    case("raytrace sums on the cpu, wrong shape and dtype", lambda e: rt(e, sums=e.torch.zeros((4, 4), dtype=e.torch.float64)))

    # Progressive and Adaptive: what they refuse about their own arguments (cast: a cast frame does not ask the scene for its depth)
    pr = lambda e, samples=4, **kw: e.sqt.Progressive(e.ds, e.cam, samples, W, H, **kw)       # noqa: E731
    case("Progressive samples 0", lambda e: pr(e, samples=0))
    case("Progressive done -1", lambda e: pr(e, done=-1))
    case("Progressive done 5 of 4", lambda e: pr(e, done=5))
    case("Progressive samples 0 and done", lambda e: pr(e, samples=0, done=5))
    case("Progressive samples 0 and bad shard", lambda e: pr(e, samples=0, shard=BAD_SHARD))
    case("Progressive done and bad shard", lambda e: pr(e, done=5, shard=BAD_SHARD))
    case("Progressive resume without sums", lambda e: pr(e, done=2, cast=True))
    case("Progressive resume without sums, oversized", lambda e: e.sqt.Progressive(e.ds, e.cam, 4, BIG, BIG, cast=True, done=2))
    ad = lambda e, samples=4, tol=0.1, **kw: e.sqt.Adaptive(e.ds, e.cam, samples, W, H, tol, **kw)   # noqa: E731
    case("Adaptive samples 0", lambda e: ad(e, samples=0))
    case("Adaptive tol -1", lambda e: ad(e, tol=-1))
    case("Adaptive tol nan", lambda e: ad(e, tol=float("nan")))
    case("Adaptive eps -1", lambda e: ad(e, eps=-1))
    case("Adaptive first 0", lambda e: ad(e, first=0))
    case("Adaptive step 0", lambda e: ad(e, step=0))
    case("Adaptive done 9 of 4", lambda e: ad(e, done=9))
    case("Adaptive rule not callable", lambda e: ad(e, rule=5))
    case("Adaptive resume without tensors", lambda e: ad(e, done=2))
    case("Adaptive resume with sums only", lambda e: ad(e, done=2, sums=np.zeros((W, H, 3), np.float32)))
    case("Adaptive samples 0 and tol", lambda e: ad(e, samples=0, tol=-1))
    case("Adaptive tol and first", lambda e: ad(e, tol=-1, first=0))
    case("Adaptive first and done", lambda e: ad(e, first=0, done=9))
    case("Adaptive done and rule", lambda e: ad(e, done=9, rule=5))
    case("Adaptive rule and resume", lambda e: ad(e, rule=5, done=2))
    case("Adaptive resume and bad shard", lambda e: ad(e, done=2, shard=BAD_SHARD))

    # the denoiser's parameters and denoise= of render_adaptive
    case("make_params unknown", lambda e: e.dn.make_params(sigma_p=1.0, foo=1, bar=2))
    case("make_params no sigma_p", lambda e: e.dn.make_params(passes=3))
    case("make_params form", lambda e: e.dn.make_params(sigma_p=1.0, form="fast"))
    case("make_params unknown and no sigma_p", lambda e: e.dn.make_params(foo=1))
    case("make_params no sigma_p and form", lambda e: e.dn.make_params(form="fast"))
    for what, v in (("str", "yes"), ("0", 0), ("-1.0", -1.0), ("False", False), ("None", None), ("list", [4.0])):
        case(f"denoise_options {what}", lambda e, v=v: e.R.denoise_options(v))

    # render_*: what is refused before anything is uploaded (bih = None: the upload is never reached)
    rp = lambda e, step=1, **kw: next(e.R.render_progressive(None, e.cam, 4, (W, H), step, **kw))     # noqa: E731
    case("render_progressive step 0", lambda e: rp(e, step=0))
    case("render_progressive depth 0", lambda e: rp(e, depth=0))
    case("render_progressive depth float", lambda e: rp(e, depth=3.0))
    case("render_progressive sky two numbers", lambda e: rp(e, sky=(1, 2)))
    case("render_progressive sky a number", lambda e: rp(e, sky=5))
    case("render_progressive step and depth", lambda e: rp(e, step=0, depth=0))
    case("render_progressive depth and sky", lambda e: rp(e, depth=True, sky="x"))
    ra = lambda e, tol=0.1, **kw: next(e.R.render_adaptive(None, e.cam, 4, (W, H), tol, **kw))         # noqa: E731
    case("render_adaptive first 0", lambda e: ra(e, first=0))
    case("render_adaptive step 0", lambda e: ra(e, step=0))
    case("render_adaptive tol -1", lambda e: ra(e, tol=-1))
    case("render_adaptive eps nan", lambda e: ra(e, eps=float("nan")))
    case("render_adaptive depth 9", lambda e: ra(e, depth=9))
    case("render_adaptive sky four numbers", lambda e: ra(e, sky=(1, 2, 3, 4)))
    case("render_adaptive denoise str", lambda e: ra(e, denoise="x"))
    case("render_adaptive first and tol", lambda e: ra(e, first=0, tol=-1))
    case("render_adaptive tol and depth", lambda e: ra(e, tol=-1, depth=9))
    case("render_adaptive depth and sky", lambda e: ra(e, depth=9, sky=5))
    case("render_adaptive sky and denoise", lambda e: ra(e, sky=5, denoise="x"))
    rv = lambda e, cams=None, **kw: e.R.render_views_rgb8(None, [e.cam] if cams is None else cams, 4, (W, H), **kw)   # noqa: E731
    case("render_views_rgb8 no camera", lambda e: rv(e, cams=[]))
    case("render_views_rgb8 depth bool", lambda e: rv(e, depth=False))
    case("render_views_rgb8 sky bad down", lambda e: rv(e, sky=((1, 2, 3), (1, 2))))
    case("render_views_rgb8 no camera and depth", lambda e: rv(e, cams=[], depth=0))
    case("render_views_rgb8 depth and sky", lambda e: rv(e, depth=0, sky=5))

    # the denoiser, handed something that is not on a device
    img = lambda e, *shape, **kw: e.torch.zeros(shape, **kw)                                    # noqa: E731
    case("denoise cpu color", lambda e: e.dn.denoise(img(e, W, H, 3), None, None, None, sigma_p=1.0))
    case("denoise numpy color", lambda e: e.dn.denoise(np.zeros((W, H, 3), np.float32), None, None, None, sigma_p=1.0))
    case("denoise cpu color and no sigma_p", lambda e: e.dn.denoise(img(e, W, H, 3), None, None, None))
    case("denoise_variance cpu counts", lambda e: e.dn.denoise_variance(None, None, img(e, W, H, dtype=e.torch.int32)))
    case("denoise_variance counts a list", lambda e: e.dn.denoise_variance(None, None, [[1, 2]]))
    return c


# ---- the "gpu" group ------------------------------------------------------------------------------------------------------
def _gpu_cases():
    c = []

    def case(name, fn):
        c.append(("gpu:" + name, fn))

    F, I, U = "float32", "int32", "uint8"
    rng = lambda e, sums, **kw: e.ds.render_rows_range(e.cam, SAMPLES, W, H, 0, 1, sums, **kw)                  # noqa: E731
    msk = lambda e, sums, **kw: e.ds.render_rows_masked(e.cam, SAMPLES, W, H, 0, 1, sums, **kw)                 # noqa: E731
    vws = lambda e, sums, **kw: e.ds.render_views([e.cam, e.cam], SAMPLES, W, H, sums=sums, **kw)               # noqa: E731
    for kind in WRONG:
        case(f"render_rows_range sums {kind}", lambda e, k=kind: rng(e, e.wrong(k, (W, H, 3), F)))
        case(f"render_rows_masked sums {kind}", lambda e, k=kind: msk(e, e.wrong(k, (W, H, 3), F)))
        case(f"render_rows_masked mask {kind}", lambda e, k=kind: msk(e, e.t((W, H, 3)), mask=e.wrong(k, (W, H), U)))
        case(f"render_rows_masked sums2 {kind}", lambda e, k=kind: msk(e, e.t((W, H, 3)), sums2=e.wrong(k, (W, H, 3), F)))
        case(f"render_rows_masked counts {kind}", lambda e, k=kind: msk(e, e.t((W, H, 3)), counts=e.wrong(k, (W, H), I)))
        case(f"render_views sums {kind}", lambda e, k=kind: vws(e, e.wrong(k, (2, W, H, 3), F)))
        case(f"intersect out.tri {kind}", lambda e, k=kind: e.ds.intersect(RAYS, RAYS, out=(e.wrong(k, (4,), I), None, None)))
        case(f"intersect out.dist {kind}", lambda e, k=kind: e.ds.intersect(RAYS, RAYS, out=(None, e.wrong(k, (4,), F), None)))
        case(f"intersect out.point {kind}", lambda e, k=kind: e.ds.intersect(RAYS, RAYS, out=(None, None, e.wrong(k, (4, 3), F))))
        case(f"raytrace sums {kind}", lambda e, k=kind: e.ds.raytrace(RAYS, RAYS, sums=e.wrong(k, (4, 3), F)))
        case(f"adaptive_update sums {kind}",
             lambda e, k=kind: e.ds.adaptive_update(e.wrong(k, (W, H, 3), F), e.t((W, H, 3)), e.t((W, H), I), e.t((W, H), U), 0.1, 1.0))
        case(f"adaptive_update counts {kind}",
             lambda e, k=kind: e.ds.adaptive_update(e.t((W, H, 3)), e.t((W, H, 3)), e.wrong(k, (W, H), I), e.t((W, H), U), 0.1, 1.0))
    case("render_rows_range no sums", lambda e: rng(e, None))
    case("render_rows_masked no sums", lambda e: msk(e, None))
    case("render_views sums without the views", lambda e: vws(e, e.t((W, H, 3))))
    case("render_rows_range sums shape and dtype", lambda e: rng(e, e.t((W, H), "float64")))
    case("render_rows_masked sums and mask", lambda e: msk(e, e.wrong("dtype", (W, H, 3), F), mask=e.wrong("shape", (W, H), U)))
    case("render_rows_masked no sums and mask", lambda e: msk(e, None, mask=e.wrong("shape", (W, H), U)))
    case("render_rows_masked mask and sums2", lambda e: msk(e, e.t((W, H, 3)), mask=e.wrong("dtype", (W, H), U), sums2=e.wrong("shape", (W, H, 3), F)))
    case("render_rows_masked sums2 and counts", lambda e: msk(e, e.t((W, H, 3)), sums2=e.wrong("device", (W, H, 3), F), counts=e.wrong("dtype", (W, H), I)))
    case("render_rows_range bad shard and sums", lambda e: rng(e, e.wrong("shape", (W, H, 3), F), shard=BAD_SHARD))
    case("intersect out.tri and out.point", lambda e: e.ds.intersect(RAYS, RAYS, out=(e.wrong("dtype", (4,), I), None, e.wrong("shape", (4, 3), F))))
    case("intersect bad rays and out.tri", lambda e: e.ds.intersect(np.zeros((4, 2)), RAYS, out=(e.wrong("dtype", (4,), I), None, None)))
    case("adaptive_update mask dtype", lambda e: e.ds.adaptive_update(e.t((W, H, 3)), e.t((W, H, 3)), e.t((W, H), I), e.t((W, H), I), 0.1, 1.0))
    case("adaptive_update mask and sums", lambda e: e.ds.adaptive_update(e.t((W, H)), e.t((W, H, 3)), e.t((W, H), I), e.t((W, H), I), 0.1, 1.0))

    # the denoiser's images: color decides the device and the shape, the others are held to it
    def dn(e, **kw):
        a = {"color": e.t((W, H, 3)), "tri": e.t((W, H), I), "normal": e.t((W, H, 3)), "point": e.t((W, H, 3)), "sigma_p": 1.0}
        a.update(kw)
        return e.dn.denoise(a.pop("color"), a.pop("tri"), a.pop("normal"), a.pop("point"), **a)
    case("denoise color [8, 8, 4]", lambda e: dn(e, color=e.t((W, H, 4))))
    case("denoise color [8, 8]", lambda e: dn(e, color=e.t((W, H))))
    case("denoise color dtype", lambda e: dn(e, color=e.t((W, H, 3), "float64")))
    case("denoise color contiguity", lambda e: dn(e, color=e.t((W, 3, H)).permute(0, 2, 1)))
    for name, shape, dtype in (("tri", (W, H), I), ("normal", (W, H, 3), F), ("point", (W, H, 3), F), ("var", (W, H), F), ("out", (W, H, 3), F)):
        for kind in WRONG:
            case(f"denoise {name} {kind}", lambda e, n=name, s=shape, d=dtype, k=kind: dn(e, **{n: e.wrong(k, s, d)}))
        case(f"denoise {name} a numpy array", lambda e, n=name, s=shape: dn(e, **{n: np.zeros(s, np.float32)}))
    for name in ("tri", "normal", "point"):
        case(f"denoise {name} missing", lambda e, n=name: dn(e, **{n: None}))
    for kind in WRONG:
        case(f"denoise out variance {kind}", lambda e, k=kind: dn(e, var=e.t((W, H)), out=(None, e.wrong(k, (W, H), F))))
    case("denoise out variance without var", lambda e: dn(e, out=(None, e.t((W, H)))))
    case("denoise no sigma_p and tri", lambda e: dn(e, sigma_p=None, tri=e.wrong("dtype", (W, H), I)))
    case("denoise unknown parameter and tri", lambda e: dn(e, radius=3, tri=e.wrong("dtype", (W, H), I)))
    case("denoise tri and normal", lambda e: dn(e, tri=e.wrong("dtype", (W, H), I), normal=e.wrong("shape", (W, H, 3), F)))
    case("denoise point and var", lambda e: dn(e, point=e.wrong("device", (W, H, 3), F), var=e.wrong("shape", (W, H), F)))
    case("denoise var and out", lambda e: dn(e, var=e.wrong("dtype", (W, H), F), out=e.wrong("shape", (W, H, 3), F)))
    case("denoise out and out variance without var", lambda e: dn(e, out=(e.wrong("shape", (W, H, 3), F), e.t((W, H)))))
    for kind in WRONG:
        case(f"denoise_variance sums {kind}", lambda e, k=kind: e.dn.denoise_variance(e.wrong(k, (W, H, 3), F), e.t((W, H, 3)), e.t((W, H), I)))
        case(f"denoise_variance sums2 {kind}", lambda e, k=kind: e.dn.denoise_variance(e.t((W, H, 3)), e.wrong(k, (W, H, 3), F), e.t((W, H), I)))
    case("denoise_variance counts dtype", lambda e: e.dn.denoise_variance(e.t((W, H, 3)), e.t((W, H, 3)), e.t((W, H), F)))
    case("denoise_variance sums missing", lambda e: e.dn.denoise_variance(None, e.t((W, H, 3)), e.t((W, H), I)))
    case("denoise_frame unknown parameter", lambda e: e.dn.denoise_frame(e.ds, e.cam, W, H, e.t((W, H, 3)), radius=3))
    case("denoise_frame form", lambda e: e.dn.denoise_frame(e.ds, e.cam, W, H, e.t((W, H, 3)), form="fast"))

    # frame state: what a checkpoint was rendered under, and a scene that changes under a frame
    pr = lambda e, samples=SAMPLES, **kw: e.sqt.Progressive(e.ds, e.cam, samples, W, H, **kw)          # noqa: E731
    ad = lambda e, samples=SAMPLES, **kw: e.sqt.Adaptive(e.ds, e.cam, samples, W, H, 0.1, **kw)        # noqa: E731
    state = lambda e: {"sums": e.t((W, H, 3)), "sums2": e.t((W, H, 3)), "counts": e.t((W, H), I), "mask": e.torch.ones((W, H), dtype=e.torch.uint8, device=e.dev)}   # noqa: E731

    def under(e, make, depth=None, sky=None, both=False):
        """Begin a frame, change the scene under it, step; the scene is put back whatever happens."""
        f = make(e)
        try:
            if depth is not None:
                e.ds.set_depth(depth)
            if sky is not None:
                e.ds.set_sky(sky)
            f.step(1) if isinstance(f, e.sqt.Progressive) else f.step()
        finally:
            e.ds.set_depth(3)
            e.ds.set_sky(None)
    for name, make in (("Progressive", pr), ("Adaptive", ad)):
        case(f"{name} checkpoint depth 4", lambda e, make=make: make(e, depth=4))
        case(f"{name} checkpoint depth 0", lambda e, make=make: make(e, depth=0))
        case(f"{name} checkpoint depth a float", lambda e, make=make: make(e, depth=3.0))
        case(f"{name} checkpoint sky", lambda e, make=make: make(e, sky=(0.5, 0.25, 1.0)))
        case(f"{name} checkpoint sky up and down", lambda e, make=make: make(e, sky=((0.5, 0.25, 1.0), (0.0, 0.0, 0.125))))
        case(f"{name} checkpoint sky of two numbers", lambda e, make=make: make(e, sky=(1, 2)))
        case(f"{name} checkpoint depth and sky", lambda e, make=make: make(e, depth=4, sky=(0.5, 0.25, 1.0)))
        case(f"{name} bad shard and checkpoint depth", lambda e, make=make: make(e, depth=4, shard=BAD_SHARD))
        case(f"{name} depth changed under the frame", lambda e, make=make: under(e, make, depth=5))
        case(f"{name} sky changed under the frame", lambda e, make=make: under(e, make, sky=(0.5, 0.25, 1.0)))
        case(f"{name} depth and sky changed under the frame", lambda e, make=make: under(e, make, depth=5, sky=(0.5, 0.25, 1.0)))
    case("Progressive resume without sums", lambda e: pr(e, done=1))
    case("Progressive checkpoint depth and resume without sums", lambda e: pr(e, done=1, depth=4))
    case("Progressive sums shape", lambda e: pr(e, done=1, sums=np.zeros((W, H), np.float32)))
    case("Progressive sums shape of a tensor", lambda e: pr(e, sums=e.t((W + 1, H, 3))))
    case("Progressive step 0", lambda e: pr(e).step(0))
    case("Progressive finished", lambda e: pr(e, done=SAMPLES, sums=e.t((W, H, 3))).step(1))
    case("Progressive finished and step 0", lambda e: pr(e, done=SAMPLES, sums=e.t((W, H, 3))).step(0))
    for name, shape in (("sums", (W, H, 3)), ("sums2", (W, H, 3)), ("counts", (W, H)), ("mask", (W, H))):
        case(f"Adaptive {name} shape", lambda e, n=name, s=shape: ad(e, **{**state(e), n: np.zeros(s[:-1] + (s[-1] + 1,), np.float32)}))
    case("Adaptive sums2 and mask shape", lambda e: ad(e, **{**state(e), "sums2": e.t((W, H)), "mask": e.t((W,), U)}))

    def finished(e, live):
        s = state(e)
        s["counts"].fill_(SAMPLES)
        if not live:
            s["mask"].zero_()
        ad(e, done=SAMPLES, **s).step()
    case("Adaptive finished: all samples", lambda e: finished(e, True))
    case("Adaptive finished: no pixel live", lambda e: finished(e, False))
    case("Adaptive rule returns another shape", lambda e: ad(e, rule=lambda s, q, c, m: m[:4]).step())      # renders the one 8 x 8 range
    return c


CASES = {"cpu": _cpu_cases(), "gpu": _gpu_cases()}
assert len({n for g in CASES.values() for n, _ in g}) == sum(len(g) for g in CASES.values()), "case names are unique"


def outcome(fn, env):
    """[exception type, message] of a case; [None, None] for a case that raised nothing."""
    try:
        fn(env)
    except Exception as ex:                          # noqa: BLE001 -- the type is what is recorded
        return [type(ex).__name__, str(ex)]
    return [None, None]


def run(group, env):
    """case name -> [exception type, message] for every case of the group."""
    return {name: outcome(fn, env) for name, fn in CASES[group]}


def golden(group):
    """The recorded outcomes of a group: the entries of the file whose names begin with the group's."""
    with open(GOLDEN_FILE) as f:
        return {k: v for k, v in json.load(f).items() if k.startswith(group + ":")}


def check(group, env):
    """Holds the package to the file: every case of the group ran, the file holds these cases and no others of the group, and every
    case raised the recorded exception with the recorded message.  Prints what differs before it asserts."""
    want, got = golden(group), run(group, env)
    assert set(got) == set(want), sorted(set(got) ^ set(want))
    bad = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    for k, (g, w) in bad.items():
        print(f"{k}:\n   got  {g}\n   want {w}")
    assert not bad, sorted(bad)
    assert all(t is not None for t, _ in want.values())
    return len(got)


def gpu_env(sqt):
    """The "gpu" group's environment: data/scene.obj uploaded once."""
    data = os.path.join(ROOT, "data")
    return Env(sqt, sqt.DeviceScene(sqt.BIH(sqt.Mesh.from_obj(os.path.join(data, "scene.obj"), data)), 0))


if __name__ == "__main__":
    group, path = sys.argv[1], sys.argv[2]
    for p in (ROOT, os.path.join(ROOT, "oracle")):
        sys.path.insert(0, p)
    pkg = importlib.import_module("squigly-trace_amd")
    pkg.lib()
    got = run(group, gpu_env(pkg) if group == "gpu" else Env(pkg))
    silent = [k for k, (t, _) in got.items() if t is None]
    assert not silent, f"these cases raised nothing: {silent}"
    held = {}
    if os.path.exists(path):
        with open(path) as f:
            held = {k: v for k, v in json.load(f).items() if not k.startswith(group + ":")}
    held.update(got)
    with open(path, "w") as f:
        json.dump(dict(sorted(held.items())), f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(got)} {group} cases in {path}")
