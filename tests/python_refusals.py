"""The refusals of the Python layer, case by case: what tests/test_python_refusals.py and tests/test_gpu_python_refusals.py hold the
package to.  Belongs here: the named cases (each a callable that must raise), the environment they run in and the recorder; no test.

Two groups.  "cpu": everything the package refuses before it asks torch for a stream or the library for a device, on a scene that
was never uploaded (every call that gets past its refusal would fail in some other way).  "gpu": the tensor refusals and the frame
state refusals, which need a real scene and device: data/scene.obj at 8 x 8 pixels and 2 samples (on 2 sub-rays where a lens frame
is needed).  A CPU tensor stands in for "a tensor on the wrong device".  Cases with two faults at once fix which one is reported.

tests/golden/python_refusals.json holds case name -> [exception type, message].  It is a transcript of the package as it was before
its rules were gathered in one place -- the first twelve features' before _plumbing.py, those of lens, mlens, shutter, temporal and
film before the seven libraries were bound by one helper and the lens frame got one driver -- not of the package under test:

    python tests/python_refusals.py cpu tests/golden/python_refusals.json       (no GPU needed)
    python tests/python_refusals.py gpu tests/golden/python_refusals.json       (on an MI355X)

each run in a checkout of that earlier commit with this file copied into its tests/; a group replaces its own entries in the file
and leaves the other group's alone.  (Recording again on a later parent is also a check of the entries already held: they must come
out byte for byte.)"""
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
        self.LN, self.ML, self.SH, self.T, self.F = (importlib.import_module(sqt.__name__ + m) for m in (".lens", ".mlens", ".shutter", ".temporal", ".film"))
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
nan, inf = float("nan"), float("inf")
OPEN, CLOSE = ((0.0, 7.0, 0.75), (1.5, 0.0, 0.0)), ((0.5, 7.0, 0.75), (1.5, 0.0, 0.125))      # a Motion's poses: (position, angles)
LENS_CALLS = ("lens_rays", "render_lens", "render_lens_masked", "shutter_rays", "render_shutter", "render_shutter_masked")
SLOTS = 2048                                         # film.SLOTS
UNSET = object()


def motion(e, time_jitter=None):
    """A Motion; time_jitter: set on it after the constructor's check (motion_arg's own refusal)."""
    m = e.sqt.Motion(OPEN, CLOSE)
    if time_jitter is not None:
        m.time_jitter = time_jitter
    return m


def lens_call(e, name, lens=UNSET, mo=UNSET, S=8, R=4, w=W, h=H, rr=None, sums=UNSET, index=None, n_live=0, **kw):
    """One of the six lens-frame calls (LENS_CALLS) on the scene: under the camera, or -- the shutter calls -- under `mo`.  rr: the
    sub-ray range, which the listed calls take as two arguments."""
    lens = e.sqt.Lens() if lens is UNSET else lens
    head = (motion(e) if mo is UNSET else mo) if "shutter" in name else e.cam
    fn = getattr(e.ds, name)
    if name.endswith("_masked"):
        r0, r1 = (0, R) if rr is None else rr
        return fn(head, lens, S, R, w, h, r0, r1, None if sums is UNSET else sums, index, n_live, **kw)
    if sums is not UNSET:
        kw["sums"] = sums
    return fn(head, lens, S, R, w, h, r_range=rr, **kw)


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

    # ---- lens, mlens, shutter, temporal, film ----
    # Lens(...) and Motion(...): the values
    for what, kw in (("jitter a str", dict(jitter="1")), ("aperture a bool", dict(aperture=True)), ("focus None", dict(focus=None)),
                     ("jitter 1.5", dict(jitter=1.5)), ("jitter -0.1", dict(jitter=-0.1)), ("jitter nan", dict(jitter=nan)),
                     ("aperture -1", dict(aperture=-1)), ("aperture inf", dict(aperture=inf)), ("aperture nan", dict(aperture=nan)),
                     ("open aperture focus 0", dict(aperture=0.1, focus=0)), ("open aperture focus inf", dict(aperture=0.1, focus=inf)),
                     ("jitter 2 and aperture a bool", dict(jitter=2, aperture=True)), ("jitter 2 and aperture -1", dict(jitter=2, aperture=-1)),
                     ("aperture inf and focus 0", dict(aperture=inf, focus=0))):
        case(f"Lens {what}", lambda e, kw=kw: e.sqt.Lens(**kw))
    for what, v in (("a bool", True), ("a str", "1"), ("None", None), ("-0.1", -0.1), ("1.01", 1.01), ("nan", nan), ("inf", inf)):
        case(f"Motion time_jitter {what}", lambda e, v=v: e.sqt.Motion(OPEN, CLOSE, v))
    for what, v in (("None", None), ("a number", 3), ("a position of two", ((0, 0), (0, 0, 0))), ("one triple", ((0, 0, 0),)),
                    ("a str inside", ((0, 0, "x"), (0, 0, 0))), ("three triples", ((0, 0, 0),) * 3)):
        case(f"Motion open {what}", lambda e, v=v: e.sqt.Motion(v, CLOSE))
        case(f"Motion close {what}", lambda e, v=v: e.sqt.Motion(OPEN, v))
    case("Motion bad camera text", lambda e: e.sqt.Motion(b"0 7 0.75\n1.57 0", CLOSE))
    case("Motion bad camera text as str", lambda e: e.sqt.Motion(OPEN, "no camera"))
    case("Motion time_jitter and open", lambda e: e.sqt.Motion(None, CLOSE, 2))
    case("Motion open and close", lambda e: e.sqt.Motion(3, None))
    for what, v in (("a camera", lambda e: e.cam), ("None", lambda e: None), ("a tuple", lambda e: (OPEN, CLOSE)),
                    ("time_jitter nan afterwards", lambda e: motion(e, nan)), ("time_jitter 2 afterwards", lambda e: motion(e, 2.0))):
        case(f"motion_arg {what}", lambda e, v=v: e.SH.motion_arg(v(e)))

    # lens.frame_args and what follows it, through the six lens-frame calls
    for name in LENS_CALLS:
        lc = lambda e, name=name, **kw: lens_call(e, name, **kw)                                 # noqa: E731
        dense, listed, rays, shutter = not name.endswith("_masked"), name.endswith("_masked"), name.endswith("_rays"), "shutter" in name
        for what, kw in (("lens None", dict(lens=None)), ("lens a tuple", dict(lens=(1.0, 0.0, 1.0))), ("samples 0", dict(S=0)),
                         ("subrays 0", dict(R=0)), ("samples -8", dict(S=-8)), ("samples 2^31", dict(S=2 ** 31, R=1)),
                         ("subrays do not divide", dict(S=8, R=3)), ("samples a float", dict(S=8.0)), ("subrays a float", dict(R=4.0)),
                         ("samples a bool", dict(S=True, R=1)), ("range empty", dict(rr=(2, 2))), ("range negative", dict(rr=(-1, 2))),
                         ("range beyond", dict(rr=(0, 5))), ("range of floats", dict(rr=(0.0, 2))), ("range end a str", dict(rr=(0, "2"))),
                         ("bad shard", dict(shard=BAD_SHARD)), ("shard row block 0", dict(shard=(0, 0, 1))),
                         ("oversized", dict(w=BIG, h=BIG)),
                         ("lens and samples 0", dict(lens=None, S=0)), ("samples 0 and bad range", dict(S=0, rr=(2, 2))),
                         ("float samples and not dividing", dict(S=8.0, R=3)), ("not dividing and bad range", dict(R=3, rr=(0, 5))),
                         ("bad range and bad shard", dict(rr=(2, 2), shard=BAD_SHARD)), ("bad shard and oversized", dict(w=BIG, h=BIG, shard=BAD_SHARD))):
            case(f"{name} {what}", lambda e, lc=lc, kw=kw: lc(e, **kw))
        if dense:
            case(f"{name} r_range a number", lambda e, lc=lc: lc(e, rr=5))
            case(f"{name} r_range of three", lambda e, lc=lc: lc(e, rr=(0, 1, 2)))
            case(f"{name} r_range a str", lambda e, lc=lc: lc(e, rr="ab"))
        if rays:                      # (a frame's fold has no ray-slot limit of its own: its batches are planned)
            case(f"{name} ray slots", lambda e, lc=lc: lc(e, S=4096, R=4096, w=1024, h=1024, rr=(0, 2048)))
            case(f"{name} oversized and ray slots", lambda e, lc=lc: lc(e, S=4096, R=4096, w=BIG, h=BIG, rr=(0, 2048)))
        if not rays:
            for what, v in (("0", 0), ("a bool", True), ("inf", inf), ("nan", nan), ("-1", -1), ("a str", "64")):
                case(f"{name} work_mb {what}", lambda e, lc=lc, v=v: lc(e, work_mb=v))
            case(f"{name} bad range and work_mb", lambda e, lc=lc: lc(e, rr=(2, 2), work_mb=0))
            case(f"{name} work_mb and bad shard", lambda e, lc=lc: lc(e, work_mb=0, shard=BAD_SHARD))
            case(f"{name} work_mb and oversized", lambda e, lc=lc: lc(e, work_mb=0, w=BIG, h=BIG))
        if dense and not rays:
            cpu3 = lambda e: e.torch.zeros((W, H, 3))                                            # noqa: E731 -- never looked at
            case(f"{name} range from 1 without sums", lambda e, lc=lc: lc(e, rr=(1, 4)))
            case(f"{name} sum2 without sum", lambda e, lc=lc: lc(e, sums=(None, cpu3(e))))
            case(f"{name} second moments from 1 without a pair", lambda e, lc=lc: lc(e, rr=(1, 4), sums=cpu3(e), want_sum2=True))
            case(f"{name} oversized and range without sums", lambda e, lc=lc: lc(e, w=BIG, h=BIG, rr=(1, 4)))
            case(f"{name} range without sums and second moments", lambda e, lc=lc: lc(e, rr=(1, 4), want_sum2=True))
        if listed:
            for what, v in (("a float", 2.0), ("a bool", True), ("None", None), ("-1", -1), ("above the pixels", W * H + 1)):
                case(f"{name} n_live {what}", lambda e, lc=lc, v=v: lc(e, n_live=v))
            case(f"{name} sums None", lambda e, lc=lc: lc(e, n_live=4))
            case(f"{name} sums None and n_live 0", lambda e, lc=lc: lc(e))
            case(f"{name} n_live above and sums None", lambda e, lc=lc: lc(e, n_live=W * H + 1))
            case(f"{name} oversized and n_live", lambda e, lc=lc: lc(e, w=BIG, h=BIG, n_live=-1))
            case(f"{name} work_mb and n_live", lambda e, lc=lc: lc(e, work_mb=0, n_live=-1))
        if shutter:
            case(f"{name} motion a camera", lambda e, lc=lc: lc(e, mo=e.cam))
            case(f"{name} motion None", lambda e, lc=lc: lc(e, mo=None))
            case(f"{name} time_jitter nan afterwards", lambda e, lc=lc: lc(e, mo=motion(e, nan)))
            case(f"{name} motion and lens", lambda e, lc=lc: lc(e, mo=None, lens=None))
            case(f"{name} time_jitter and samples 0", lambda e, lc=lc: lc(e, mo=motion(e, -1.0), S=0))
    lp = lambda e, mask, counts, r=0: e.ds.live_pixels(mask, counts, r)                          # noqa: E731
    u8 = lambda e, *shape: e.torch.zeros(shape, dtype=e.torch.uint8)                            # noqa: E731
    case("live_pixels r_begin -1", lambda e: lp(e, u8(e, W, H), None, -1))
    case("live_pixels r_begin 2^31", lambda e: lp(e, u8(e, W, H), None, 2 ** 31))
    case("live_pixels r_begin a float", lambda e: lp(e, u8(e, W, H), None, 1.0))
    case("live_pixels r_begin a bool", lambda e: lp(e, u8(e, W, H), None, False))
    case("live_pixels neither mask nor counts", lambda e: lp(e, None, None))
    case("live_pixels mask a numpy array", lambda e: lp(e, np.zeros((W, H), np.uint8), None))
    case("live_pixels counts a list", lambda e: lp(e, None, [[1, 2]]))
    case("live_pixels mask [8]", lambda e: lp(e, u8(e, W), None))
    case("live_pixels mask [8, 8, 1]", lambda e: lp(e, u8(e, W, H, 1), None))
    case("live_pixels r_begin and neither", lambda e: lp(e, None, None, -1))
    case("live_pixels mask a list and counts fine", lambda e: lp(e, [[1]], e.torch.zeros((W, H), dtype=e.torch.int32)))

    # temporal: the parameters, Temporal's numbers and what its constructor refuses before it looks at the scene
    case("temporal make_params unknown", lambda e: e.T.make_params(sigma_p=1.0, foo=1, bar=2))
    case("temporal make_params no sigma_p", lambda e: e.T.make_params(alpha_min=0.5))
    case("temporal make_params max_history a float", lambda e: e.T.make_params(sigma_p=1.0, max_history=8.0))
    case("temporal make_params max_history a bool", lambda e: e.T.make_params(sigma_p=1.0, max_history=True))
    case("temporal make_params unknown and no sigma_p", lambda e: e.T.make_params(foo=1))
    case("temporal make_params no sigma_p and max_history", lambda e: e.T.make_params(max_history=8.0))
    numbers = (("spp 0", dict(spp=0)), ("spp a float", dict(spp=2.0)), ("spp a bool", dict(spp=True)), ("spp a str", dict(spp="2")),
               ("period 0", dict(period=0)), ("period a float", dict(period=64.0)), ("period None", dict(period=None)),
               ("max_history 0", dict(max_history=0)), ("max_history a float", dict(max_history=32.0)), ("max_history 65537", dict(max_history=65537)),
               ("spp * period 2^32", dict(spp=2 ** 20, period=2 ** 12)), ("spp * period 2^31", dict(spp=2 ** 16, period=2 ** 15)),
               ("alpha_min a bool", dict(alpha_min=True)), ("alpha_min a str", dict(alpha_min="0.1")), ("alpha_min -0.1", dict(alpha_min=-0.1)),
               ("alpha_min 1.5", dict(alpha_min=1.5)), ("alpha_min nan", dict(alpha_min=nan)), ("alpha_min None", dict(alpha_min=None)),
               ("spp and period", dict(spp=0, period=0)), ("period and max_history", dict(period=0, max_history=0)),
               ("max_history 0 and too many samples", dict(max_history=0, spp=2 ** 20, period=2 ** 12)),
               ("too many samples and max_history 65537", dict(spp=2 ** 20, period=2 ** 12, max_history=65537)),
               ("max_history 65537 and alpha_min", dict(max_history=65537, alpha_min=2)))
    ta = lambda e, spp=2, period=64, alpha_min=0.1, max_history=32: e.T._temporal_args(spp, period, alpha_min, max_history)   # noqa: E731
    tm = lambda e, spp=2, **kw: e.T.Temporal(e.ds, W, H, spp, **kw)                               # noqa: E731
    rs = lambda e, spp=2, cams=None, **kw: next(e.R.render_sequence(None, [e.cam] if cams is None else cams, spp, (W, H), **kw))   # noqa: E731
    for what, kw in numbers:
        case(f"_temporal_args {what}", lambda e, kw=kw: ta(e, **kw))
        case(f"Temporal {what}", lambda e, kw=kw: tm(e, **kw))
        case(f"render_sequence {what}", lambda e, kw=kw: rs(e, **kw))
    case("Temporal film a number", lambda e: tm(e, film=5))
    case("Temporal film the class", lambda e: tm(e, film=e.sqt.Film))
    case("Temporal frames -1", lambda e: tm(e, frames=-1))
    case("Temporal frames a float", lambda e: tm(e, frames=1.0))
    case("Temporal history without a camera", lambda e: tm(e, history=np.zeros(4, np.uint8)))
    case("Temporal camera without a history", lambda e: tm(e, camera=e.cam))
    case("Temporal spp and film", lambda e: tm(e, spp=0, film=5))
    case("Temporal film and frames", lambda e: tm(e, film=5, frames=-1))
    case("Temporal frames and history", lambda e: tm(e, frames=-1, camera=e.cam))
    case("render_sequence no camera", lambda e: rs(e, cams=[]))
    case("render_sequence film a number", lambda e: rs(e, film=5))
    case("render_sequence denoise str", lambda e: rs(e, denoise="x"))
    case("render_sequence denoise 0", lambda e: rs(e, denoise=0))
    case("render_sequence depth 0", lambda e: rs(e, depth=0))
    case("render_sequence sky two numbers", lambda e: rs(e, sky=(1, 2)))
    case("render_sequence no camera and spp", lambda e: rs(e, cams=[], spp=0))
    case("render_sequence spp and film", lambda e: rs(e, spp=0, film=5))
    case("render_sequence film and denoise", lambda e: rs(e, film=5, denoise="x"))
    case("render_sequence denoise and depth", lambda e: rs(e, denoise="x", depth=0))
    case("render_sequence depth and sky", lambda e: rs(e, depth=0, sky=5))

    # film: the meter, the curve, the parameters, the tables, Film(...) and film=
    for what, kw in (("unknown", dict(foo=1, bar=2)), ("permille 0", dict(permille=0)), ("permille 1001", dict(permille=1001)),
                     ("permille a float", dict(permille=500.0)), ("permille a bool", dict(permille=True)), ("key a str", dict(key="0.18")),
                     ("rate a bool", dict(rate=True)), ("fallback None", dict(fallback=None)), ("e_min 0", dict(e_min=0)),
                     ("e_min above e_max", dict(e_min=2.0, e_max=1.0)), ("e_max inf", dict(e_max=inf)), ("e_min nan", dict(e_min=nan)),
                     ("rate 1.5", dict(rate=1.5)), ("rate -0.1", dict(rate=-0.1)), ("rate nan", dict(rate=nan)), ("fallback 0", dict(fallback=0)),
                     ("fallback nan", dict(fallback=nan)), ("unknown and permille", dict(foo=1, permille=0)), ("permille and key", dict(permille=0, key="x")),
                     ("key and e_min", dict(key="x", e_min=0)), ("e_min and rate", dict(e_min=0, rate=2)), ("rate and fallback", dict(rate=2, fallback=0))):
        case(f"make_meter {what}", lambda e, kw=kw: e.F.make_meter(**kw))
    for what, v in (("a name it has not", "sepia"), ("5", 5), ("-1", -1), ("a float", 1.0), ("a bool", True), ("None", None)):
        case(f"curve_index {what}", lambda e, v=v: e.F.curve_index(v))
    for what, kw in (("curve", dict(curve="sepia")), ("white a str", dict(curve="reinhard", white="4")), ("white a bool", dict(white=True)),
                     ("reinhard white 0", dict(curve="reinhard", white=0)), ("reinhard white nan", dict(curve="reinhard", white=nan)),
                     ("dither 1", dict(curve="atan", dither=1)), ("dither None", dict(curve="atan", dither=None)),
                     ("reference with a table", dict(n_lut=16)), ("reference with dither", dict(dither=True)),
                     ("exposure a str", dict(curve="atan", exposure="1")), ("exposure a bool", dict(curve="atan", exposure=True)),
                     ("curve and white", dict(curve="sepia", white="4")), ("white and dither", dict(curve="reinhard", white=0, dither=1)),
                     ("dither and reference", dict(dither=1)), ("reference with a table and exposure", dict(n_lut=16, exposure="1"))):
        case(f"film make_params {what}", lambda e, kw=kw: e.F.make_params(**kw))
    for what, v in (("1", 1), ("65537", 65537), ("a float", 16.0), ("a bool", True), ("None", None)):
        case(f"srgb_lut n {what}", lambda e, v=v: e.F.srgb_lut(v))
        case(f"gamma_lut n {what}", lambda e, v=v: e.F.gamma_lut(2.2, v))
    for what, v in (("0", 0), ("-1", -1), ("inf", inf), ("nan", nan), ("a str", "2.2"), ("a bool", True)):
        case(f"gamma_lut g {what}", lambda e, v=v: e.F.gamma_lut(v))
    case("gamma_lut g and n", lambda e: e.F.gamma_lut(0, 1))
    for what, kw in (("table [4, 4]", dict(curve="atan", lut=np.zeros((4, 4), np.float32))), ("table of one entry", dict(curve="atan", lut=[0.5])),
                     ("table of 65537 entries", dict(curve="atan", lut=np.zeros(65537, np.float32))), ("table a scalar", dict(curve="atan", lut=0.5)),
                     ("auto True", dict(auto=True)), ("auto a list", dict(auto=[("key", 0.18)])), ("auto unknown", dict(auto={"foo": 1})),
                     ("auto rate 2", dict(auto={"rate": 2})), ("curve", dict(curve="sepia")), ("reference with a table", dict(lut=np.zeros(16, np.float32))),
                     ("reference with dither", dict(dither=True)), ("exposure a str", dict(curve="atan", exposure="1")),
                     ("table and curve", dict(curve="sepia", lut=[0.5])), ("curve and auto", dict(curve="sepia", auto=True)),
                     ("white and auto", dict(curve="reinhard", white=0, auto=True))):
        case(f"Film {what}", lambda e, kw=kw: e.sqt.Film(**kw))
    case("Film exposure_state a str", lambda e: setattr(e.sqt.Film(), "exposure_state", "1"))
    for what, v in (("a number", 5), ("a str", "film"), ("the class", lambda e: e.sqt.Film), ("a dict", {})):
        case(f"film_arg {what}", lambda e, v=v: e.F.film_arg(v(e) if callable(v) else v))
    for what, v in (("a numpy array", lambda e: np.zeros((W, H, 3), np.float32)), ("None", lambda e: None), ("a list", lambda e: [[[0.0] * 3]]),
                    ("a cpu tensor", lambda e: e.torch.zeros((W, H, 3))), ("a cpu tensor [3]", lambda e: e.torch.zeros(3)),
                    ("a cpu tensor [8, 8, 4] float64", lambda e: e.torch.zeros((W, H, 4), dtype=e.torch.float64))):
        case(f"histogram color {what}", lambda e, v=v: e.F.histogram(v(e)))
        case(f"develop color {what}", lambda e, v=v: e.F.develop(v(e)))
        case(f"Film() of {what}", lambda e, v=v: e.sqt.Film()(v(e)))
    case("expose hist a numpy array", lambda e: e.F.expose(np.zeros(SLOTS, np.int32)))
    case("expose hist None", lambda e: e.F.expose(None))
    case("expose hist a cpu tensor", lambda e: e.F.expose(e.torch.zeros(SLOTS, dtype=e.torch.int32)))
    case("expose unknown meter and hist", lambda e: e.F.expose(None, foo=1))
    case("expose rate 2 and hist", lambda e: e.F.expose(None, rate=2))
    case("develop color and curve", lambda e: e.F.develop(None, curve="sepia"))

    # AdaptiveLens: what its constructor refuses before it looks at the scene
    al = lambda e, lens=UNSET, S=8, R=4, tol=0.1, **kw: e.sqt.AdaptiveLens(e.ds, e.cam, e.sqt.Lens() if lens is UNSET else lens, S, R, W, H, tol, **kw)   # noqa: E731
    for what, kw in (("lens None", dict(lens=None)), ("samples 0", dict(S=0)), ("subrays 0", dict(R=0)), ("subrays do not divide", dict(R=3)),
                     ("samples a float", dict(S=8.0)), ("lens and samples", dict(lens=None, S=0))):
        case(f"AdaptiveLens {what}", lambda e, kw=kw: al(e, **kw))
    case("AdaptiveLens motion a camera", lambda e: al(e, motion=e.cam))
    case("AdaptiveLens motion a number", lambda e: al(e, motion=5))
    case("AdaptiveLens time_jitter nan afterwards", lambda e: al(e, motion=motion(e, nan)))
    case("AdaptiveLens lens and motion", lambda e: al(e, lens=None, motion=5))
    case("AdaptiveLens checkpoint under a motion, frame under none", lambda e: al(e, checkpoint_motion=motion(e)))
    case("AdaptiveLens checkpoint under none, frame under a motion", lambda e: al(e, motion=motion(e), checkpoint_motion=None))
    case("AdaptiveLens checkpoint under another motion", lambda e: al(e, motion=motion(e), checkpoint_motion=e.sqt.Motion(OPEN, CLOSE, 0.5)))
    case("AdaptiveLens motion and checkpoint motion", lambda e: al(e, motion=5, checkpoint_motion=None))
    case("AdaptiveLens checkpoint motion and tol", lambda e: al(e, checkpoint_motion=motion(e), tol=-1))
    case("AdaptiveLens tol -1", lambda e: al(e, tol=-1))
    case("AdaptiveLens eps nan", lambda e: al(e, eps=nan))
    case("AdaptiveLens first 0", lambda e: al(e, first=0))
    case("AdaptiveLens step 0", lambda e: al(e, step=0))
    case("AdaptiveLens done 5 of 4 sub-rays", lambda e: al(e, done=5))
    case("AdaptiveLens rule not callable", lambda e: al(e, rule=5))
    case("AdaptiveLens resume without tensors", lambda e: al(e, done=2))
    case("AdaptiveLens subrays and tol", lambda e: al(e, R=3, tol=-1))
    case("AdaptiveLens done and rule", lambda e: al(e, done=5, rule=5))
    case("AdaptiveLens resume and bad shard", lambda e: al(e, done=2, shard=BAD_SHARD))
    case("AdaptiveLens bad shard", lambda e: al(e, shard=BAD_SHARD))
    case("AdaptiveLens oversized", lambda e: e.sqt.AdaptiveLens(e.ds, e.cam, e.sqt.Lens(), 8, 4, BIG, BIG, 0.1))
    case("AdaptiveLens oversized wavefront", lambda e: e.sqt.AdaptiveLens(e.ds, e.cam, e.sqt.Lens(), 8, 4, WAVE[0], WAVE[1], 0.1))
    case("AdaptiveLens bad shard and oversized", lambda e: e.sqt.AdaptiveLens(e.ds, e.cam, e.sqt.Lens(), 8, 4, BIG, BIG, 0.1, shard=BAD_SHARD))

    # render_lens_rgb8, render_adaptive(lens= / subrays= / motion= / film=): every check that precedes the upload
    rl = lambda e, samples=8, **kw: e.R.render_lens_rgb8(None, e.cam, samples, (W, H), **kw)      # noqa: E731
    for what, kw in (("lens a number", dict(lens=5)), ("samples 0", dict(samples=0)), ("subrays do not divide", dict(subrays=3)),
                     ("subrays a float", dict(subrays=4.0)), ("motion a camera", dict(motion=UNSET)), ("motion a number", dict(motion=5)),
                     ("depth 0", dict(depth=0)), ("depth a float", dict(subrays=4, depth=3.0)), ("sky two numbers", dict(sky=(1, 2))),
                     ("lens and motion", dict(lens=5, motion=5)), ("subrays and motion", dict(subrays=3, motion=5)),
                     ("motion and depth", dict(motion=5, depth=0)), ("depth and sky", dict(depth=0, sky=5))):
        case(f"render_lens_rgb8 {what}", lambda e, kw=kw: rl(e, **{k: (e.cam if v is UNSET else v) for k, v in kw.items()}))
    case("render_lens_rgb8 time_jitter nan afterwards", lambda e: rl(e, motion=motion(e, nan)))
    case("render_lens_rgb8 time_jitter and sky", lambda e: rl(e, motion=motion(e, nan), sky="x"))
    ral = lambda e, samples=8, tol=0.1, first=2, step=2, **kw: next(e.R.render_adaptive(None, e.cam, samples, (W, H), tol, first=first, step=step, **kw))   # noqa: E731
    ln = lambda e: e.sqt.Lens()                                                                  # noqa: E731
    case("render_adaptive film a number", lambda e: ral(e, film=5, denoise=True))
    case("render_adaptive film without denoise", lambda e: ral(e, film=e.sqt.Film()))
    case("render_adaptive film with denoise False", lambda e: ral(e, film=e.sqt.Film(), denoise=False))
    case("render_adaptive film a number and first 0", lambda e: ral(e, film=5, first=0))
    case("render_adaptive film without denoise and tol", lambda e: ral(e, film=e.sqt.Film(), tol=-1))
    case("render_adaptive film without denoise, with a lens", lambda e: ral(e, film=e.sqt.Film(), lens=ln(e), subrays=4))
    case("render_adaptive subrays without a lens", lambda e: ral(e, subrays=4))
    case("render_adaptive motion without a lens", lambda e: ral(e, motion=motion(e)))
    case("render_adaptive first 0 and subrays without a lens", lambda e: ral(e, first=0, subrays=4))
    case("render_adaptive tol and motion without a lens", lambda e: ral(e, tol=-1, motion=5))
    case("render_adaptive lens a number", lambda e: ral(e, lens=5))
    case("render_adaptive lens, motion a number", lambda e: ral(e, lens=ln(e), subrays=4, motion=5))
    case("render_adaptive lens, time_jitter nan afterwards", lambda e: ral(e, lens=ln(e), subrays=4, motion=motion(e, nan)))
    case("render_adaptive lens and cast", lambda e: ral(e, lens=ln(e), subrays=4, cast=True))
    case("render_adaptive lens, subrays do not divide", lambda e: ral(e, lens=ln(e), subrays=3))
    case("render_adaptive lens, samples 0", lambda e: ral(e, samples=0, lens=ln(e)))
    case("render_adaptive lens, first no multiple", lambda e: ral(e, lens=ln(e), subrays=4, first=3))
    case("render_adaptive lens, step no multiple", lambda e: ral(e, lens=ln(e), subrays=4, step=5))
    case("render_adaptive lens, depth 9", lambda e: ral(e, lens=ln(e), subrays=4, depth=9))
    case("render_adaptive lens, sky four numbers", lambda e: ral(e, lens=ln(e), subrays=4, sky=(1, 2, 3, 4)))
    case("render_adaptive lens, denoise str", lambda e: ral(e, lens=ln(e), subrays=4, denoise="x"))
    case("render_adaptive lens: motion and cast", lambda e: ral(e, lens=ln(e), subrays=4, motion=5, cast=True))
    case("render_adaptive lens: cast and lens a number", lambda e: ral(e, lens=5, cast=True))
    case("render_adaptive lens: subrays and first", lambda e: ral(e, lens=ln(e), subrays=3, first=3))
    case("render_adaptive lens: first and depth", lambda e: ral(e, lens=ln(e), subrays=4, first=3, depth=9))
    case("render_adaptive lens: depth and sky", lambda e: ral(e, lens=ln(e), subrays=4, depth=9, sky=5))
    case("render_adaptive lens: sky and denoise", lambda e: ral(e, lens=ln(e), subrays=4, sky=5, denoise="x"))
    case("render_adaptive lens: film a number and lens a number", lambda e: ral(e, lens=5, film=5, denoise=True))
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

    # ---- lens, mlens, shutter: the frame's tensors (2 samples on 2 sub-rays) ----
    f3, i2 = (lambda e: e.t((W, H, 3))), (lambda e: e.t((W, H), I))
    for name in ("render_lens", "render_shutter"):
        lc = lambda e, name=name, **kw: lens_call(e, name, S=SAMPLES, R=2, **kw)                 # noqa: E731
        for kind in WRONG:
            case(f"{name} sums {kind}", lambda e, lc=lc, k=kind: lc(e, sums=e.wrong(k, (W, H, 3), F)))
            case(f"{name} sums2 {kind}", lambda e, lc=lc, k=kind: lc(e, sums=(f3(e), e.wrong(k, (W, H, 3), F))))
        case(f"{name} sums a numpy array", lambda e, lc=lc: lc(e, sums=np.zeros((W, H, 3), np.float32)))
        case(f"{name} sums and sums2", lambda e, lc=lc: lc(e, sums=(e.wrong("dtype", (W, H, 3), F), e.wrong("shape", (W, H, 3), F))))
        case(f"{name} bad shard and sums", lambda e, lc=lc: lc(e, sums=e.wrong("shape", (W, H, 3), F), shard=BAD_SHARD))
        case(f"{name} range without sums and sums2", lambda e, lc=lc: lc(e, rr=(1, 2), sums=(None, e.wrong("shape", (W, H, 3), F))))
    for name in ("render_lens_masked", "render_shutter_masked"):
        # (every case is wrong in something: a listed call with nothing wrong and n_live = 0 returns without a word)
        lc = lambda e, name=name, **kw: lens_call(e, name, S=SAMPLES, R=2, **{"sums": f3(e), "index": e.t((W * H,), I), "n_live": 4, **kw})   # noqa: E731
        for kind in WRONG:
            case(f"{name} sums {kind}", lambda e, lc=lc, k=kind: lc(e, sums=e.wrong(k, (W, H, 3), F)))
            case(f"{name} sums2 {kind}", lambda e, lc=lc, k=kind: lc(e, sums2=e.wrong(k, (W, H, 3), F)))
            case(f"{name} counts {kind}", lambda e, lc=lc, k=kind: lc(e, counts=e.wrong(k, (W, H), I)))
            case(f"{name} out_avg {kind}", lambda e, lc=lc, k=kind: lc(e, out_avg=e.wrong(k, (W, H, 3), F)))
            case(f"{name} out_rgb {kind}", lambda e, lc=lc, k=kind: lc(e, out_rgb=e.wrong(k, (W, H, 3), U)))
        case(f"{name} index int64", lambda e, lc=lc: lc(e, index=e.t((W * H,), "int64")))
        case(f"{name} index too short", lambda e, lc=lc: lc(e, index=e.t((3,), I)))
        case(f"{name} index on the cpu", lambda e, lc=lc: lc(e, index=e.t((W * H,), I, device="cpu")))
        case(f"{name} index [8, 8]", lambda e, lc=lc: lc(e, index=e.t((W, H), I)))
        case(f"{name} index strided", lambda e, lc=lc: lc(e, index=e.t((2 * W * H,), I)[::2]))
        case(f"{name} index a numpy array", lambda e, lc=lc: lc(e, index=np.zeros(W * H, np.int32)))
        case(f"{name} index None and n_live 0", lambda e, lc=lc: lc(e, index=None, n_live=0))
        case(f"{name} sums and sums2", lambda e, lc=lc: lc(e, sums=e.wrong("dtype", (W, H, 3), F), sums2=e.wrong("shape", (W, H, 3), F)))
        case(f"{name} sums2 and counts", lambda e, lc=lc: lc(e, sums2=e.wrong("device", (W, H, 3), F), counts=e.wrong("dtype", (W, H), I)))
        case(f"{name} counts and out_avg", lambda e, lc=lc: lc(e, counts=e.wrong("shape", (W, H), I), out_avg=e.wrong("dtype", (W, H, 3), F)))
        case(f"{name} out_avg and out_rgb", lambda e, lc=lc: lc(e, out_avg=e.wrong("shape", (W, H, 3), F), out_rgb=e.wrong("dtype", (W, H, 3), U)))
        case(f"{name} out_rgb and index", lambda e, lc=lc: lc(e, out_rgb=e.wrong("dtype", (W, H, 3), U), index=None))
        case(f"{name} bad shard and sums", lambda e, lc=lc: lc(e, sums=e.wrong("shape", (W, H, 3), F), shard=BAD_SHARD))
    lp = lambda e, mask, counts, r=0: e.ds.live_pixels(mask, counts, r)                          # noqa: E731
    for kind in ("dtype", "contiguity", "device"):           # (a mask of another shape is a frame of that shape)
        case(f"live_pixels mask {kind}", lambda e, k=kind: lp(e, e.wrong(k, (W, H), U), None))
        case(f"live_pixels counts alone {kind}", lambda e, k=kind: lp(e, None, e.wrong(k, (W, H), I), 1))
    for kind in WRONG:
        case(f"live_pixels counts {kind}", lambda e, k=kind: lp(e, e.t((W, H), U), e.wrong(k, (W, H), I), 1))
    case("live_pixels mask [8, 8, 3]", lambda e: lp(e, e.t((W, H, 3), U), None))
    case("live_pixels mask and counts", lambda e: lp(e, e.wrong("dtype", (W, H), U), e.wrong("dtype", (W, H), I)))
    case("live_pixels r_begin and mask", lambda e: lp(e, e.wrong("dtype", (W, H), U), None, -1))

    # ---- temporal.accumulate and unpack: color decides the device and the shape, the others are held to it ----
    class G:                                         # anything with .tri, .normal, .point
        def __init__(self, e, **kw):
            self.tri, self.normal, self.point = kw.get("tri", i2(e)), kw.get("normal", f3(e)), kw.get("point", f3(e))

    def acc(e, **kw):
        a = {"color": f3(e), "var": e.t((W, H)), "prev_cam": None, "prev": None, "sigma_p": 1.0}
        a.update({k: v for k, v in kw.items() if k not in ("tri", "normal", "point")})
        if "nxt" not in a:
            a["nxt"] = e.T.history(W, H, e.dev)
        g = G(e, **kw)
        return e.T.accumulate(a.pop("color"), a.pop("var"), g, a.pop("prev_cam"), a.pop("prev"), a.pop("nxt"), **a)
    need = lambda e: e.T.history_bytes(W, H)                                                     # noqa: E731
    case("accumulate color [8, 8, 4]", lambda e: acc(e, color=e.t((W, H, 4))))
    case("accumulate color [8, 8]", lambda e: acc(e, color=e.t((W, H))))
    case("accumulate color on the cpu", lambda e: acc(e, color=e.t((W, H, 3), device="cpu")))
    case("accumulate color a numpy array", lambda e: acc(e, color=np.zeros((W, H, 3), np.float32)))
    case("accumulate color dtype", lambda e: acc(e, color=e.t((W, H, 3), "float64")))
    case("accumulate color contiguity", lambda e: acc(e, color=e.t((W, 3, H)).permute(0, 2, 1)))
    for name, shape, dtype in (("var", (W, H), F), ("tri", (W, H), I), ("normal", (W, H, 3), F), ("point", (W, H, 3), F), ("alpha", (W, H), F)):
        for kind in WRONG:
            case(f"accumulate {name} {kind}", lambda e, n=name, s=shape, d=dtype, k=kind: acc(e, **{n: e.wrong(k, s, d)}))
        case(f"accumulate {name} a numpy array", lambda e, n=name, s=shape: acc(e, **{n: np.zeros(s, np.float32)}))
    case("accumulate var None", lambda e: acc(e, var=None))
    for name in ("prev", "nxt"):
        cam = (lambda e: e.cam) if name == "prev" else (lambda e: None)
        case(f"accumulate {name} a byte longer", lambda e, n=name, cam=cam: acc(e, prev_cam=cam(e), **{n: e.t((need(e) + 1,), U)}))
        case(f"accumulate {name} a byte shorter", lambda e, n=name, cam=cam: acc(e, prev_cam=cam(e), **{n: e.t((need(e) - 1,), U)}))
        case(f"accumulate {name} int8", lambda e, n=name, cam=cam: acc(e, prev_cam=cam(e), **{n: e.t((need(e),), "int8")}))
        case(f"accumulate {name} float32", lambda e, n=name, cam=cam: acc(e, prev_cam=cam(e), **{n: e.t((need(e) // 4,), F)}))
        case(f"accumulate {name} strided", lambda e, n=name, cam=cam: acc(e, prev_cam=cam(e), **{n: e.wrong("contiguity", (need(e),), U)}))
        case(f"accumulate {name} on the cpu", lambda e, n=name, cam=cam: acc(e, prev_cam=cam(e), **{n: e.t((need(e),), U, device="cpu")}))
    case("accumulate nxt None", lambda e: acc(e, nxt=None))
    case("accumulate prev without prev_cam", lambda e: acc(e, prev=e.T.history(W, H, e.dev)))
    case("accumulate prev_cam without prev", lambda e: acc(e, prev_cam=e.cam))
    case("accumulate out of four", lambda e: acc(e, out=(f3(e), e.t((W, H)), i2(e), i2(e))))
    for i, (name, shape, dtype) in enumerate((("colour", (W, H, 3), F), ("variance", (W, H), F), ("length", (W, H), I))):
        for kind in WRONG:
            case(f"accumulate out {name} {kind}",
                 lambda e, i=i, s=shape, d=dtype, k=kind: acc(e, out=tuple(e.wrong(k, s, d) if j == i else None for j in range(3))))
    case("accumulate unknown parameter and var", lambda e: acc(e, radius=3, var=e.wrong("dtype", (W, H), F)))
    case("accumulate no sigma_p and var", lambda e: acc(e, sigma_p=None, var=e.wrong("dtype", (W, H), F)))
    case("accumulate color [8, 8] and no sigma_p", lambda e: acc(e, color=e.t((W, H)), sigma_p=None))
    case("accumulate var and tri", lambda e: acc(e, var=e.wrong("dtype", (W, H), F), tri=e.wrong("shape", (W, H), I)))
    case("accumulate point and alpha", lambda e: acc(e, point=e.wrong("device", (W, H, 3), F), alpha=e.wrong("shape", (W, H), F)))
    case("accumulate alpha and prev without prev_cam", lambda e: acc(e, alpha=e.wrong("dtype", (W, H), F), prev=e.T.history(W, H, e.dev)))
    case("accumulate prev without prev_cam and a bad prev", lambda e: acc(e, prev=e.t((3,), U)))
    case("accumulate prev and nxt", lambda e: acc(e, prev_cam=e.cam, prev=e.t((3,), U), nxt=e.t((5,), U)))
    case("accumulate nxt and out of four", lambda e: acc(e, nxt=e.t((5,), U), out=(None,) * 4))
    case("accumulate out colour and variance", lambda e: acc(e, out=(e.wrong("shape", (W, H, 3), F), e.wrong("dtype", (W, H), F))))
    case("unpack hist a numpy array", lambda e: e.T.unpack(np.zeros(8, np.uint8), W, H))
    case("unpack hist on the cpu", lambda e: e.T.unpack(e.t((need(e),), U, device="cpu"), W, H))
    case("unpack hist a byte longer", lambda e: e.T.unpack(e.t((need(e) + 1,), U), W, H))
    case("unpack hist int8", lambda e: e.T.unpack(e.t((need(e),), "int8"), W, H))
    case("unpack hist strided", lambda e: e.T.unpack(e.wrong("contiguity", (need(e),), U), W, H))
    case("unpack hist of another frame", lambda e: e.T.unpack(e.T.history(W, H, e.dev), W, H + 1))
    case("unpack 0 rows", lambda e: e.T.unpack(e.T.history(W, H, e.dev), 0, H))
    case("unpack 46341 x 46341", lambda e: e.T.unpack(e.T.history(W, H, e.dev), BIG, BIG))
    case("history 0 columns", lambda e: e.T.history(W, 0, e.dev))

    # ---- film: histogram, expose, develop ----
    colors = (("[8, 8, 4]", lambda e: e.t((W, H, 4))), ("[3]", lambda e: e.t((3,))), ("float64", lambda e: e.t((W, H, 3), "float64")),
              ("strided", lambda e: e.t((W, 3, H)).permute(0, 2, 1)), ("on the cpu", lambda e: e.t((W, H, 3), device="cpu")),
              ("[0, 8, 3]", lambda e: e.t((0, H, 3))), ("[8, 0, 3]", lambda e: e.t((W, 0, 3))))
    for what, v in colors:
        case(f"histogram color {what}", lambda e, v=v: e.F.histogram(v(e)))
        case(f"develop color {what}", lambda e, v=v: e.F.develop(v(e)))
    case("Film() of color float64", lambda e: e.sqt.Film()(e.t((W, H, 3), "float64")))
    hist = lambda e: e.t((SLOTS,), I)                                                            # noqa: E731
    for kind in WRONG:
        case(f"histogram out {kind}", lambda e, k=kind: e.F.histogram(f3(e), out=e.wrong(k, (SLOTS,), I)))
        case(f"expose hist {kind}", lambda e, k=kind: e.F.expose(e.wrong(k, (SLOTS,), I)))
        case(f"develop out image {kind}", lambda e, k=kind: e.F.develop(f3(e), out=e.wrong(k, (W, H, 3), U)))
        case(f"develop out display {kind}", lambda e, k=kind: e.F.develop(f3(e), out=(None, e.wrong(k, (W, H, 3), F)), want_display=True))
    for kind in ("dtype", "contiguity", "device"):           # (a table of another length is another table)
        case(f"develop lut {kind}", lambda e, k=kind: e.F.develop(f3(e), curve="atan", lut=e.wrong(k, (16,), F)))
    case("develop lut [4, 4]", lambda e: e.F.develop(f3(e), curve="atan", lut=e.t((4, 4))))
    for kind in ("shape", "dtype", "device"):                # (a tensor of one element is contiguous whatever its stride)
        case(f"expose prev {kind}", lambda e, k=kind: e.F.expose(hist(e), prev=e.wrong(k, (1,), F)))
        case(f"expose out {kind}", lambda e, k=kind: e.F.expose(hist(e), out=e.wrong(k, (1,), F)))
        case(f"develop exposure tensor {kind}", lambda e, k=kind: e.F.develop(f3(e), exposure=e.wrong(k, (1,), F)))
    case("histogram out a numpy array", lambda e: e.F.histogram(f3(e), out=np.zeros(SLOTS, np.int32)))
    case("histogram color and out", lambda e: e.F.histogram(e.t((W, H, 4)), out=e.wrong("dtype", (SLOTS,), I)))
    case("expose unknown meter and hist", lambda e: e.F.expose(e.wrong("dtype", (SLOTS,), I), foo=1))
    case("expose hist and prev", lambda e: e.F.expose(e.wrong("dtype", (SLOTS,), I), prev=e.wrong("shape", (1,), F)))
    case("expose prev and out", lambda e: e.F.expose(hist(e), prev=e.wrong("dtype", (1,), F), out=e.wrong("shape", (1,), F)))
    case("develop exposure tensor [1, 1]", lambda e: e.F.develop(f3(e), exposure=e.t((1, 1))))
    case("develop lut of one entry", lambda e: e.F.develop(f3(e), curve="atan", lut=e.t((1,))))
    case("develop lut of 65537 entries", lambda e: e.F.develop(f3(e), curve="atan", lut=e.t((65537,))))
    case("develop lut a numpy array", lambda e: e.F.develop(f3(e), curve="atan", lut=np.zeros(16, np.float32)))
    case("develop lut under the reference curve", lambda e: e.F.develop(f3(e), lut=e.t((16,))))
    case("develop curve", lambda e: e.F.develop(f3(e), curve="sepia"))
    case("develop dither 1", lambda e: e.F.develop(f3(e), curve="atan", dither=1))
    case("develop out a pair without want_display", lambda e: e.F.develop(f3(e), out=(e.t((W, H, 3), U), f3(e))))
    case("develop out of three", lambda e: e.F.develop(f3(e), out=(None, None, None), want_display=True))
    case("develop out image a numpy array", lambda e: e.F.develop(f3(e), out=np.zeros((W, H, 3), np.uint8)))
    case("develop color and exposure tensor", lambda e: e.F.develop(e.t((W, H, 4)), exposure=e.t((2,))))
    case("develop exposure tensor and lut", lambda e: e.F.develop(f3(e), curve="atan", exposure=e.t((2,)), lut=e.t((1,))))
    case("develop lut and curve", lambda e: e.F.develop(f3(e), curve="sepia", lut=e.t((1,))))
    case("develop curve and out", lambda e: e.F.develop(f3(e), curve="sepia", out=e.wrong("dtype", (W, H, 3), U)))
    case("develop out a pair and out image", lambda e: e.F.develop(f3(e), out=(e.wrong("dtype", (W, H, 3), U), f3(e))))
    case("develop out image and display", lambda e: e.F.develop(f3(e), out=(e.wrong("dtype", (W, H, 3), U), e.wrong("shape", (W, H, 3), F)), want_display=True))

    # ---- AdaptiveLens and Temporal: frame state ----
    al = lambda e, samples=SAMPLES, **kw: e.sqt.AdaptiveLens(e.ds, e.cam, e.sqt.Lens(), samples, 2, W, H, 0.1, **kw)    # noqa: E731
    case("AdaptiveLens checkpoint depth 4", lambda e: al(e, depth=4))
    case("AdaptiveLens checkpoint depth 0", lambda e: al(e, depth=0))
    case("AdaptiveLens checkpoint depth a float", lambda e: al(e, depth=3.0))
    case("AdaptiveLens checkpoint sky", lambda e: al(e, sky=(0.5, 0.25, 1.0)))
    case("AdaptiveLens checkpoint sky up and down", lambda e: al(e, sky=((0.5, 0.25, 1.0), (0.0, 0.0, 0.125))))
    case("AdaptiveLens checkpoint sky of two numbers", lambda e: al(e, sky=(1, 2)))
    case("AdaptiveLens checkpoint depth and sky", lambda e: al(e, depth=4, sky=(0.5, 0.25, 1.0)))
    case("AdaptiveLens bad shard and checkpoint depth", lambda e: al(e, depth=4, shard=BAD_SHARD))
    case("AdaptiveLens checkpoint motion and depth", lambda e: al(e, checkpoint_motion=motion(e), depth=4))
    case("AdaptiveLens depth changed under the frame", lambda e: under(e, al, depth=5))
    case("AdaptiveLens sky changed under the frame", lambda e: under(e, al, sky=(0.5, 0.25, 1.0)))
    case("AdaptiveLens depth and sky changed under the frame", lambda e: under(e, al, depth=5, sky=(0.5, 0.25, 1.0)))
    case("AdaptiveLens under a motion, depth changed under the frame", lambda e: under(e, lambda e: al(e, motion=motion(e)), depth=5))
    for name, shape in (("sums", (W, H, 3)), ("sums2", (W, H, 3)), ("counts", (W, H)), ("mask", (W, H))):
        case(f"AdaptiveLens {name} shape", lambda e, n=name, s=shape: al(e, **{**state(e), n: np.zeros(s[:-1] + (s[-1] + 1,), np.float32)}))

    def finished_lens(e, live):
        s = state(e)
        s["counts"].fill_(2)
        if not live:
            s["mask"].zero_()
        al(e, done=2, **s).step()
    case("AdaptiveLens finished: all sub-rays", lambda e: finished_lens(e, True))
    case("AdaptiveLens finished: no pixel live", lambda e: finished_lens(e, False))
    case("AdaptiveLens rule returns another shape", lambda e: al(e, rule=lambda s, q, c, m: m[:4]).step())   # renders one 8 x 8 step of one sub-ray
    tm = lambda e, **kw: e.T.Temporal(e.ds, W, H, SAMPLES, **kw)                                  # noqa: E731

    def under_sequence(e, depth=None, sky=None):
        t = tm(e)
        try:
            if depth is not None:
                e.ds.set_depth(depth)
            if sky is not None:
                e.ds.set_sky(sky)
            t.step(e.cam)
        finally:
            e.ds.set_depth(3)
            e.ds.set_sky(None)
    case("Temporal history of another shape", lambda e: tm(e, history=np.zeros(5, np.uint8), camera=e.cam))
    case("Temporal history [2, n]", lambda e: tm(e, history=np.zeros((2, need(e)), np.uint8), camera=e.cam))
    case("Temporal checkpoint depth 4", lambda e: tm(e, depth=4))
    case("Temporal checkpoint depth 0", lambda e: tm(e, depth=0))
    case("Temporal checkpoint sky", lambda e: tm(e, sky=(0.5, 0.25, 1.0)))
    case("Temporal checkpoint depth and sky", lambda e: tm(e, depth=4, sky=(0.5, 0.25, 1.0)))
    case("Temporal denoise str", lambda e: tm(e, denoise="x"))
    case("Temporal denoise unknown parameter", lambda e: tm(e, denoise={"radius": 3}))
    case("Temporal denoise and checkpoint depth", lambda e: tm(e, denoise="x", depth=4))
    case("Temporal checkpoint depth and history", lambda e: tm(e, depth=4, history=np.zeros(5, np.uint8), camera=e.cam))
    case("Temporal depth changed under the sequence", lambda e: under_sequence(e, depth=5))
    case("Temporal sky changed under the sequence", lambda e: under_sequence(e, sky=(0.5, 0.25, 1.0)))
    case("Temporal depth and sky changed under the sequence", lambda e: under_sequence(e, depth=5, sky=(0.5, 0.25, 1.0)))
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
