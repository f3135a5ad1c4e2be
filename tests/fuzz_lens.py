"""Randomised parity campaign for the lens, shutter and temporal libraries and for DeviceScene.guides, on the random scenes and cameras
of fuzz_features.case(seed): the join between those scenes and the restatements the three libraries are held to on the room
(lens_restatement LR, shutter_restatement SHR, mlens_restatement MR, temporal_restatement, with sky_restatement SR under them).

Seed N is fuzz_features.case(N) -- scene, both cameras, w, h, shard, depth, live mask, knobs, slots, deep -- and everything new comes
from a generator of its own, default_rng([N, 3]) ([N, 1] is fuzz_features', [N, 2] fuzz_sky's), in this order (recorded seeds keep
reproducing only while it stays):

    1. S from SAMPLES (1 half as often as the others); R: one draw u -- u < 0.2: 1, u < 0.5: S, else a uniform choice among the
       divisors of S
    2. the point the range [0, R) is split at, in [1, R) (R > 1 only)
    3. the jitter's kind (0, 1, a uniform draw) and the uniform draw
    4. the aperture's kind (closed / open) and its uniform draw (times scale); the focus: a uniform draw in [0.25, 2) times the
       distance from the camera to the scene's centre (the scale where the camera sits there)
    5. the odd-lens draw and which of the four odd lenses (an aperture of 3e38 or 1e-30, or, with the aperture opened if it was
       closed, a focus of 1e-30 or 3e38)
    6. the close pose's kind (the open pose / a small step / the second camera's numbers), the step's six normal draws, time_jitter
    7. whether the seed has its sky (SR.fuzz_sky(N)) or none
    8. whether the dense frame's workspace is small, and how many whole sub-rays of the shard fit into the small one, in [1, R)
    9. the temporal call's drawn alpha_min, max_history and per-pixel alpha, then its two stops: sigma_p (the scene's default, fifty
       times that, or inf) and cos_n (0.9, 0 or -1) -- under the defaults few of these frames find history in the second camera's

Expected values come only from the restatements over the case's oracle tree (c.ob, c.flat); a case's walks are made once and
shared.  tests/test_fuzz_lens.py pins the restatements to the oracle on every seed of the pytest slice and judges what the slice
covers, without a GPU; tests/test_gpu_fuzz_lens.py runs the slice.  Every comparison is on bits with NaN = NaN, RGB8 exactly.

    python tests/fuzz_lens.py [seconds=240] [first_seed=0]

prints one line per mismatch with the seed that reproduces it, and a summary."""
import ctypes as C
import functools
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)
import pyoracle as O  # noqa: E402

import fuzz_features as FF  # noqa: E402
import fuzz_gpu as F  # noqa: E402
import lens_restatement as LR  # noqa: E402
import mlens_restatement as MR  # noqa: E402
import shutter_restatement as SHR  # noqa: E402
import sky_restatement as SR  # noqa: E402
import temporal_restatement as TR  # noqa: E402
from bitcmp import canon, same  # noqa: E402

sqt = FF.sqt
lens_lib = importlib.import_module("squigly-trace_amd.lens")
denoise_lib = importlib.import_module("squigly-trace_amd.denoise")
f32 = np.float32
N = 400
SLICE = range(1000, 1000 + N)                 # the pytest slice: tests/test_fuzz_lens.py judges it, tests/test_gpu_fuzz_lens.py runs it
SAMPLES = (1, 2, 3, 4, 6, 8)
SAMPLE_WEIGHTS = np.array([1, 2, 2, 2, 2, 2]) / 11
ODD_LENSES = ("aperture 3e38", "aperture 1e-30", "focus 1e-30", "focus 3e38")
SENT = {"sum": 5.5, "sum2": -6.5, "count": 77, "avg": 8.25, "rgb": 99}       # run_sky_case's sentinels
NORMAL_ATOL = 1e-6                                                         # test_guides_are_the_oracles' tolerance of the normal


def camera_numbers(text):
    """(pos, angles) of a camera file of fuzz_gpu.make_camera: each decimal as the float32 nearest to it (strtof), which is how the
    oracle's camera reads the file -- test_fuzz_lens.py's pin of the still motion says so on every seed."""
    strtof = C.CDLL(None).strtof
    strtof.restype, strtof.argtypes = C.c_float, [C.c_char_p, C.c_void_p]
    v = [float(strtof(t, None)) for t in text.split()]
    assert len(v) == 6
    return tuple(v[:3]), tuple(v[3:])


def case(seed):
    c = FF.case(seed)
    rng = np.random.default_rng([seed, 3])
    pixels = len(c.rows) * c.h
    # 1. samples and sub-rays
    c.S = int(rng.choice(SAMPLES, p=SAMPLE_WEIGHTS))
    u = rng.random()
    divisors = [r for r in range(1, c.S + 1) if c.S % r == 0]
    c.R = 1 if u < 0.2 else c.S if u < 0.5 else int(rng.choice(divisors))
    # 2. the two ranges
    c.split = int(rng.integers(1, c.R)) if c.R > 1 else None
    c.ranges = [(0, c.R)] if c.split is None else [(0, c.split), (c.split, c.R)]
    # 3. jitter
    kind, ju = int(rng.integers(0, 3)), rng.random()
    jitter = (0.0, 1.0, float(f32(ju)))[kind]
    # 4. aperture and focus
    p0, a0 = camera_numbers(c.camt)
    is_open, au = rng.random() < 0.6, rng.uniform(0.01, 0.5)
    aperture = float(f32(au * c.scale)) if is_open else 0.0
    dist = float(np.linalg.norm(np.array(p0)))
    focus = float(min(f32(rng.uniform(0.25, 2.0) * (dist if dist > 0 else c.scale)), f32(3e38)))       # (inf is no focus)
    # 5. odd lenses
    c.odd = None
    odd, which = rng.random(), int(rng.integers(0, 4))
    if odd < 0.1:
        c.odd = ODD_LENSES[which]
        if which < 2:
            aperture = float(f32((3e38, 1e-30)[which]))
        else:
            focus = float(f32((1e-30, 3e38)[which - 2]))
            aperture = aperture if aperture > 0 else float(f32(au * c.scale))
    c.lens = (jitter, aperture, focus)
    # 6. the motion
    p2, a2 = camera_numbers(c.camt2)
    mkind, step, tj = int(rng.integers(0, 3)), rng.normal(0, 1, 6), float(rng.choice([0.0, 0.5, 1.0]))
    if mkind == 0:
        p1, a1 = p0, a0
    elif mkind == 1:
        p1 = tuple(float(f32(p + 0.1 * c.scale * s)) for p, s in zip(p0, step[:3]))
        a1 = tuple(float(f32(a + 0.1 * s)) for a, s in zip(a0, step[3:]))
    else:
        p1, a1 = p2, a2
    c.motion_kind = ("still", "step", "second camera")[mkind]
    c.motion, c.still, c.time_jitter = (p0, a0, p1, a1), (p0, a0, p0, a0), tj
    # 7. the sky
    c.sky = SR.fuzz_sky(seed) if rng.random() < 0.5 else None
    # 8. the workspace: None, or the bytes of `fit` whole sub-rays of the shard as MiB (a binary fraction: work_mb * 2^20 is them again)
    small, fit = rng.random() < 0.7, int(rng.integers(1, c.R)) if c.R > 1 else None
    c.fit = fit if small and fit is not None else None
    c.work_mb = None if c.fit is None else lens_lib.work_bytes(pixels, c.fit) / 2 ** 20
    # 9. the temporal call's parameters
    c.alpha_min = float(f32(rng.choice([0.0, 0.05, 0.25, 1.0])))
    c.max_history = int(rng.choice([1, 2, 8, 65536]))
    c.alpha = rng.random((c.w, c.h)).astype(f32)
    c.alpha[rng.random((c.w, c.h)) < 0.2] = 1.0
    c.sigma_scale = float(rng.choice([1.0, 50.0, np.inf]))
    c.cos_n = float(rng.choice([0.9, 0.0, -1.0]))
    c.pixels = pixels
    return c


def batches(c):
    """The batches lens.workspace's arithmetic gives the dense frame of the case under c.work_mb: lens.plan of what `sized` hands
    the library.  With c.fit whole sub-rays fitting there are ceil(R / fit) of them."""
    return lens_lib.plan(c.pixels, 0, c.R, lens_lib.workspace(c.work_mb)(c.pixels, c.R))


# ---- expected values: every walk of a case is made once ---------------------------------------------------------------------
def cached(fn):
    @functools.wraps(fn)
    def get(c, *args):
        store = c.__dict__.setdefault("_lens_cache", {})
        key = (fn.__name__,) + args
        if key not in store:
            store[key] = fn(c, *args)
        return store[key]
    return get


def shard_pixels(c):
    """The whole frame's pixel numbers of the shard's pixels, in the shard's order."""
    return np.array([y * c.h + x for y in c.rows for x in range(c.h)], np.int64)


@cached
def rays(c, which):
    """(o [R, w * h, 3], d, seeds [R, w * h]) of the whole frame: which = "lens" (LR.rays under the first camera) or "shutter"
    (SHR.rays under the motion)."""
    if which == "lens":
        return LR.rays(c.ocam, c.lens, c.S, c.R, c.w, c.h)
    return SHR.rays(c.motion, c.time_jitter, c.lens, c.S, c.R, c.w, c.h)


def shard_rays(c, which, r_range=None):
    r0, r1 = (0, c.R) if r_range is None else r_range
    return tuple(a[r0:r1][:, shard_pixels(c)] for a in rays(c, which))


@cached
def trails(c, which):
    """The walks of the shard's sub-rays, misses kept and to the largest depth: one walk serves every depth and sky."""
    if which == "lens":
        return LR.trails(c.ob, c.flat, c.ocam, c.lens, c.S, c.R, c.w, c.h, rows=c.rows)
    return SHR.trails(c.ob, c.flat, c.motion, c.time_jitter, c.lens, c.S, c.R, c.w, c.h, rows=c.rows)


@cached
def parts(c, which):
    """s_r [R, pixels, 3] at the case's depth and sky."""
    return LR.sub_ray_sums(trails(c, which), c.depth, c.sky)


@cached
def frame(c, which):
    """(sum, sum2, avg, rgb), each [rows, h, 3], of the dense frame at the case's depth and sky."""
    s, q, avg = LR.fold(parts(c, which), c.S)
    shape = (len(c.rows), c.h, 3)
    return s.reshape(shape), q.reshape(shape), avg.reshape(shape), LR.tonemap(avg).reshape(shape)


def masked_frame(c, which, index):
    """The five buffers of the listed frame over the case's two ranges, from the sentinels: MR.indexed_fold per range."""
    n = c.pixels
    st = {"sum": np.full((n, 3), SENT["sum"], f32), "sum2": np.full((n, 3), SENT["sum2"], f32), "count": np.full(n, SENT["count"], np.int32),
          "avg": np.full((n, 3), SENT["avg"], f32), "rgb": np.full((n, 3), SENT["rgb"], np.uint8)}
    for r0, r1 in c.ranges:
        MR.indexed_fold(parts(c, which)[r0:r1][:, index], index, c.S // c.R, r0, r1, st)
    return st


def triangle_tables(c):
    """Per triangle of the oracle's flat tree: unit normal, surf, emissive *^ emit -- numpy's cross and norm in float32, operation
    for operation what DeviceScene.guides gathers from."""
    if not hasattr(c, "_tables"):
        t = c.flat
        with np.errstate(all="ignore"):
            nrm = np.cross(t["b"] - t["a"], t["c"] - t["a"]).astype(f32)
            nrm = nrm / np.sqrt((nrm * nrm).sum(-1, keepdims=True), dtype=f32)
            c._tables = (nrm.astype(f32), np.asarray(t["surf"], f32), (t["emissive"][:, None] * t["emit"]).astype(f32))
    return c._tables


PREVIOUS = ("second", "close")      # the cameras a temporal step of the first camera's frame looks back to


def camera_of(c, which):
    """The oracle's Camera of the case: "first", "second", or "close" -- the pose of the case's motion as its shutter closes
    (the first camera again, a small step from it, or about the second camera: most frames find their history under it)."""
    return {"first": lambda: c.ocam, "second": lambda: c.ocam2, "close": lambda: SHR.camera(c.motion, 1.0)}[which]()


@cached
def guides(c, which):
    """dict: tri [w, h], point, normal, surf, emit [w, h, 3] of the whole frame's first hits under camera_of(c, which); zeros where a
    ray hits nothing."""
    cam = camera_of(c, which)
    g = dict(tri=np.full((c.w, c.h), -1, np.int32), point=np.zeros((c.w, c.h, 3), f32), normal=np.zeros((c.w, c.h, 3), f32),
             surf=np.zeros((c.w, c.h, 3), f32), emit=np.zeros((c.w, c.h, 3), f32))
    nrm, surf, emit = triangle_tables(c)
    for y in range(c.w):
        for x in range(c.h):
            hit = c.ob.intersect(*O.make_ray(c.w, c.h, y, x, cam))
            if hit.hit:
                g["tri"][y, x] = hit.tri
                g["point"][y, x] = (hit.point.x, hit.point.y, hit.point.z)
                g["normal"][y, x], g["surf"][y, x], g["emit"][y, x] = nrm[hit.tri], surf[hit.tri], emit[hit.tri]
    return g


def product_camera(ocam):
    """The product's Camera with the numbers of an oracle's."""
    pos, rot = TR.camera(ocam)
    cam = sqt.Camera()
    cam.pos[:], cam.rot[:] = [float(v) for v in pos], [float(v) for v in rot]
    return cam


def sigma_p(c, factor=1.0):
    """factor times the scene's default plane-distance stop; where that is no number (a scene with a NaN vertex has NaN bounds,
    inf * 0) the stop of a scene of the case's scale: the library refuses a NaN."""
    s = factor * denoise_lib.default_sigma_p(FF.product_bih(c).bounds)
    return s if s == s else 0.02 * c.scale


def temporal_params(c, drawn):
    """(alpha, keyword parameters) of the temporal call: the defaults, or the case's drawn ones."""
    if drawn:
        return c.alpha, dict(sigma_p=sigma_p(c, c.sigma_scale), alpha_min=c.alpha_min, max_history=c.max_history, cos_n=c.cos_n)
    return None, dict(sigma_p=sigma_p(c))


def temporal_want(c, previous, before, now, drawn, g_before=None, g_now=None):
    """(the first block of the frame under the camera `previous`, the result of accumulating the first camera's frame on it) on
    host arrays: before, now = (colour, variance) of the two frames; the guides default to the oracle's."""
    g0, g1 = g_before or guides(c, previous), g_now or guides(c, "first")
    alpha, params = temporal_params(c, drawn)
    first = TR.accumulate(*before, g0["tri"], g0["normal"], g0["point"], None, None)
    return first, TR.accumulate(*now, g1["tri"], g1["normal"], g1["point"], camera_of(c, previous), first["block"], alpha=alpha, **params)


# ---- one case on the GPU -----------------------------------------------------------------------------------------------------
def differ(got, want):
    """How many pixels (rows of three) differ, NaN = NaN."""
    return int((canon(np.asarray(got)).reshape(-1, 3) != canon(np.asarray(want)).reshape(-1, 3)).any(-1).sum())


def run_case(seed):
    """Every check of the seed; returns the list of mismatch messages (empty: all equal).  A refusal is a mismatch."""
    import torch
    F.load_libraries()
    temporal = importlib.import_module("squigly-trace_amd.temporal")
    if FF.DEVICE_ERROR:
        raise RuntimeError(f"not run: the device reported an error earlier in this process ({FF.DEVICE_ERROR[0]})")
    c = case(seed)
    bad = []
    cam, cam2 = sqt.camera_from_text(c.camt), sqt.camera_from_text(c.camt2)
    w, h, S, R, shard = c.w, c.h, c.S, c.R, c.shard
    rows = len(c.rows)
    shape = (rows, h, 3)
    dev = "cuda:0"
    lens = sqt.Lens(*c.lens)
    motion = sqt.Motion((c.motion[0], c.motion[1]), (c.motion[2], c.motion[3]), c.time_jitter)
    heads = (("lens", cam), ("shutter", motion))
    ds = sqt.DeviceScene(FF.product_bih(c), 0)

    def call(which, form):
        return getattr(ds, {"rays": "%s_rays", "dense": "render_%s", "masked": "render_%s_masked"}[form] % which)

    def host(t):
        return t.cpu().numpy()

    def rays_check(what, got, want):
        torch.cuda.synchronize()
        o, d, s = (host(t) for t in got)
        nb = want[0].shape[0]
        if o.shape[0] != nb or o.reshape(nb, -1, 3).shape != want[0].shape:
            bad.append(f"{what}: shape {o.shape}")
        elif not (same(o.reshape(want[0].shape), want[0]) and same(d.reshape(want[1].shape), want[1])):
            bad.append(f"{what}: {differ(o, want[0])} origins and {differ(d, want[1])} directions of {want[2].size} differ")
        elif not np.array_equal(s.reshape(want[2].shape), want[2]):
            bad.append(f"{what}: seeds differ")

    def frame_check(what, got, want):
        torch.cuda.synchronize()
        for name, g, e in zip(("sum", "sum2", "avg"), got[:3], want[:3]):
            if not same(host(g), e):
                bad.append(f"{what}: {name} differs in {differ(host(g), e)}/{rows * h} pixels")
                return
        if not np.array_equal(host(got[3]), want[3]):
            bad.append(f"{what}: rgb8 differs")

    try:
        for k, val in c.knobs.items():
            ds.set_option(k, val)
        ds.set_option("slots", c.slots)                                 # from the start: a workspace only grows
        ds.set_option("deep", c.deep)
        ds.set_depth(c.depth)
        if c.sky is not None:
            ds.set_sky(*c.sky)
        if c.fit is not None and len(batches(c)) != -(-R // c.fit):
            bad.append(f"work_mb {c.work_mb}: {len(batches(c))} batches planned, {-(-R // c.fit)} expected")
        for which, head in heads:
            # ---- 1. the rays: the whole frame, a drawn range of the shard, the shard
            rays_check(f"{which}_rays, whole frame", call(which, "rays")(head, lens, S, R, w, h), rays(c, which))
            rays_check(f"{which}_rays, shard {shard}", call(which, "rays")(head, lens, S, R, w, h, shard=shard), shard_rays(c, which))
            rr = c.ranges[-1]
            rays_check(f"{which}_rays, shard {shard}, sub-rays {rr}", call(which, "rays")(head, lens, S, R, w, h, shard=shard, r_range=rr),
                       shard_rays(c, which, rr))
            # ---- 2. the dense frame: one call, the two ranges, the small workspace; and variant 1
            want = frame(c, which)
            render = call(which, "dense")
            for variant in (2, 1):
                ds.set_option("variant", variant)
                what = f"render_{which} {S}/{R} lens {c.lens}, depth {c.depth}, variant {variant}"
                one = render(head, lens, S, R, w, h, shard=shard, want_sum2=True)
                frame_check(f"{what}, one call", one, want)
                first = render(head, lens, S, R, w, h, shard=shard, r_range=c.ranges[0], want_sum2=True)
                if len(c.ranges) > 1:
                    first = render(head, lens, S, R, w, h, shard=shard, r_range=c.ranges[1], sums=(first.sum, first.sum2))
                frame_check(f"{what}, ranges {c.ranges}", first, want)
                small = render(head, lens, S, R, w, h, shard=shard, want_sum2=True, work_mb=c.work_mb)
                frame_check(f"{what}, work_mb {c.work_mb}", small, want)
                if not all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for o in (first, small) for a, b in zip(one, o)):
                    bad.append(f"{what}: the one call, the ranges and the small workspace differ from each other in their bits")
            ds.set_option("variant", 2)
            # ---- 3. the listed frame over the two ranges
            live = c.live
            mask = torch.from_numpy(live.astype(np.uint8)).to(dev)
            B = {"sum": torch.full(shape, SENT["sum"], dtype=torch.float32, device=dev),
                 "sum2": torch.full(shape, SENT["sum2"], dtype=torch.float32, device=dev),
                 "count": torch.full((rows, h), SENT["count"], dtype=torch.int32, device=dev),
                 "avg": torch.full(shape, SENT["avg"], dtype=torch.float32, device=dev),
                 "rgb": torch.full(shape, SENT["rgb"], dtype=torch.uint8, device=dev)}
            want_index = MR.live_list(live.reshape(-1).astype(np.uint8), None, 0)
            for r0, r1 in c.ranges:
                index, n_live = ds.live_pixels(mask, B["count"], r0)
                n = int(n_live.item())
                if n != len(want_index) or not np.array_equal(host(index)[:n], want_index):
                    bad.append(f"live_pixels at r_begin {r0}: the list differs from mlens_restatement.live_list")
                    break
                call(which, "masked")(head, lens, S, R, w, h, r0, r1, B["sum"], index, n, sums2=B["sum2"], counts=B["count"], shard=shard,
                                      out_avg=B["avg"], out_rgb=B["rgb"])
            else:
                torch.cuda.synchronize()
                st = masked_frame(c, which, want_index)
                got = {k: host(t).reshape(st[k].shape) for k, t in B.items()}
                flat_live = live.reshape(-1)
                dense = [a.reshape(-1, 3) for a in want]
                if not (same(got["sum"], st["sum"]) and same(got["sum2"], st["sum2"]) and np.array_equal(got["count"], st["count"])
                        and same(got["avg"], st["avg"]) and np.array_equal(got["rgb"], st["rgb"])):
                    bad.append(f"render_{which}_masked over {c.ranges}: sum, sum2, count, avg or rgb differs from mlens_restatement")
                if not (same(got["sum"][flat_live], dense[0][flat_live]) and same(got["sum2"][flat_live], dense[1][flat_live])
                        and (got["count"][flat_live] == R).all() and same(got["avg"][flat_live], dense[2][flat_live])
                        and np.array_equal(got["rgb"][flat_live], dense[3][flat_live])):
                    bad.append(f"render_{which}_masked over {c.ranges}: a live pixel differs from the dense frame's restatement")
                dead = ~flat_live
                if not all((got[k][dead] == SENT[k]).all() for k in SENT):
                    bad.append(f"render_{which}_masked over {c.ranges}: a dead pixel lost a sentinel")
        # ---- 4. the guides under the first and second camera and the motion's close pose: the whole frame, and the first's shard
        cams = {"first": cam, "second": cam2, "close": product_camera(camera_of(c, "close"))}
        G = {}
        for name, cm in cams.items():
            g, want = ds.guides(cm, w, h), guides(c, name)
            torch.cuda.synchronize()
            G[name] = g
            for field in ("tri", "point", "normal", "surf", "emit"):
                got, exp = host(getattr(g, field)), want[field]
                if not (np.array_equal(got, exp) if field == "tri" else same(got, exp)):
                    bad.append(f"guides under the {name} camera: {field} differs")
            hit = want["tri"] >= 0
            if not np.allclose(host(g.normal)[hit], want["normal"][hit], atol=NORMAL_ATOL, equal_nan=True):
                bad.append(f"guides under the {name} camera: a normal is further than {NORMAL_ATOL} from the oracle's")
            if host(g.normal)[~hit].any() or host(g.surf)[~hit].any() or host(g.emit)[~hit].any():
                bad.append(f"guides under the {name} camera: a pixel without a hit has a normal, a surf or an emit")
        g, want = ds.guides(cam, w, h, shard=shard), guides(c, "first")
        torch.cuda.synchronize()
        for field in ("tri", "point", "normal", "surf", "emit"):
            got, exp = host(getattr(g, field)), want[field][c.rows]
            if not (np.array_equal(got, exp) if field == "tri" else same(got, exp)):
                bad.append(f"guides of the shard {shard}: {field} differs")
        # ---- 5. temporal: the frame of a previous camera as the first block, the first camera's frame accumulated on it
        ones = torch.full((w, h), c.spp, dtype=torch.int32, device=dev)
        frames = {}
        for name, cm in cams.items():                                   # colour and variance: a masked call and denoise_variance
            sums, sums2 = (torch.zeros((w, h, 3), dtype=torch.float32, device=dev) for _ in range(2))
            avg = torch.empty((w, h, 3), dtype=torch.float32, device=dev)
            ds.render_rows_masked(cm, c.spp, w, h, 0, c.spp, sums, sums2=sums2, out_avg=avg)
            frames[name] = (avg, denoise_lib.denoise_variance(sums, sums2, ones))
        torch.cuda.synchronize()
        on_host = {name: tuple(host(t) for t in fr) for name, fr in frames.items()}
        g_host = {name: {f: host(getattr(g, f)) for f in ("tri", "normal", "point")} for name, g in G.items()}
        color1, var1 = frames["first"]

        def temporal_check(what, got, blk, want):
            torch.cuda.synchronize()
            for name, a, e in (("colour", got[0], want["color"]), ("variance", got[1], want["var"])):
                if not same(host(a), e):
                    bad.append(f"{what}: {name} differs in {int((canon(host(a)) != canon(e)).sum())} values")
            if not np.array_equal(host(got[2]), want["len"]):
                bad.append(f"{what}: length differs")
            hist = temporal.unpack(blk, w, h)
            torch.cuda.synchronize()
            for name in TR.BLOCK_FIELDS:
                a, e = host(getattr(hist, name)), want["block"][name]
                if not (same(a, e) if e.dtype == f32 else np.array_equal(a, e)):
                    bad.append(f"{what}: the block's {name} differs")

        for previous in PREVIOUS:
            blk0 = temporal.history(w, h, 0)
            out0 = temporal.accumulate(*frames[previous], G[previous], None, None, blk0, sigma_p=sigma_p(c))
            for drawn in (False, True):
                alpha, params = temporal_params(c, drawn)
                first, want = temporal_want(c, previous, on_host[previous], on_host["first"], drawn, g_host[previous], g_host["first"])
                if not drawn:
                    temporal_check(f"temporal, the first block under the {previous} camera", out0, blk0, first)
                what = f"temporal.accumulate on the {previous} camera's block, {'drawn' if drawn else 'default'} parameters"
                d_alpha = None if alpha is None else torch.from_numpy(alpha).to(dev)
                nxt = temporal.history(w, h, 0)
                got = temporal.accumulate(color1, var1, G["first"], cams[previous], blk0, nxt, alpha=d_alpha, **params)
                temporal_check(what, got, nxt, want)
                nxt = temporal.history(w, h, 0)
                col, var = color1.clone(), var1.clone()
                got = temporal.accumulate(col, var, G["first"], cams[previous], blk0, nxt, alpha=d_alpha, out=(col, var), **params)
                temporal_check(what + ", in place", got, nxt, want)
    except sqt.SquiglyError as e:
        if " failed: " in str(e):                                       # a HIP error is no refusal: nothing more runs on this device
            FF.DEVICE_ERROR.append(f"seed {seed}: {e}")
            raise
        bad.append(f"refused: {e}")
    except RuntimeError as e:                                           # torch's own report of a HIP error (a synchronize, a copy)
        if "HIP error" in str(e) or "CUDA error" in str(e):
            FF.DEVICE_ERROR.append(f"seed {seed}: {e}")
        raise
    finally:
        ds.close()
    return bad


def describe(c):
    return (f"seed {c.seed}: {len(c.v)} tris, {c.w}x{c.h}, shard {c.shard}, S {c.S} R {c.R} ranges {c.ranges}, lens {c.lens} ({c.odd}), "
            f"motion {c.motion_kind} tj {c.time_jitter}, sky {c.sky}, depth {c.depth}, work_mb {c.work_mb} (fit {c.fit}), deep {c.deep}, "
            f"slots {c.slots}, {c.knobs}")


def main(budget=240.0, seed=0):
    return F.campaign("fuzz_lens", run_case, budget, seed)


if __name__ == "__main__":
    sys.exit(main(float(sys.argv[1]) if len(sys.argv) > 1 else 240.0, int(sys.argv[2]) if len(sys.argv) > 2 else 0))
