"""Randomised parity campaign for the image stages -- the denoiser's variance and a-trous filter, sparse frames (mask and upsample),
the glare pyramid and the film library -- and for the drivers that chain them (denoise_frame, render_sparse, Temporal(sparse=,
denoise=, film=), Film(auto=, glare=, balance=)), on the random scenes and cameras of fuzz_features.case(seed): the join between
those scenes and the restatements the four kernel families are held to on hand-made inputs and the room (denoise_restatement DNR,
upsample_restatement UR, glare_restatement GR, film_restatement FR).

Seed N is fuzz_features.case(N) -- scene, both cameras, scale, live mask, depth, knobs -- and everything new comes from a generator
of its own, default_rng([N, 4]) ([N, 1] is fuzz_features', [N, 2] fuzz_sky's, [N, 3] fuzz_lens', [N, 5] test_fuzz_level1's), in this
order (recorded seeds keep reproducing only while it stays):

    1. the image: per side one draw u (u < 0.5: the case's own side, 1..16) and one of BIG_SIDES; where rows * cols > PIXEL_CAP the
       larger side falls back to the case's.  c.w, c.h become the image's "w rows by h columns" (the case's own stay in c.case_w,
       c.case_h), the shard the whole frame
    2. the close camera: six normal draws, a step of 0.1 * scale and 0.1 rad from the first camera's numbers (fuzz_lens' close pose,
       from this generator).  The case then takes, of "first", "second" and "close", the camera whose oracle frame has the most
       pixels with a hit and a 4-neighbour without one (ties: the earlier); the other two are c.previous
    3. the guide poison: one draw (< 0.25: poisoned), how many pixels (2..6), and per pixel a uniform draw (which pixel, among the
       hit pixels where there are any), a kind (a NaN normal component, a zero normal, an infinite point component, tri = -1) and
       a component
    4. the masked render: spp from 1..4, one draw u and one split point j in [1, spp) (u < 0.5: the split is 1), and a uniform
       image: < 0.2 a pixel is live in neither range, < 0.5 in the first only, else in both
    5. k in -24..24: the colour of glare and film is avg * 2^k
    6. the filter: passes (PASS_WEIGHTS), sigma_l, eps_l, the factor on the scene's sigma_p, normal_squarings in 0..8
    7. the sparse frame: stride in 1..16, offset (oy, ox) in [0, s)^2, cos_n, the factor on sigma_p
    8. the glare: whether the exposure is a number or a device float, the exposure (10^u, u in -2..2), three gains (GAINS,
       GAIN_WEIGHTS), threshold, ceiling (kept above the threshold), levels (LEVEL_WEIGHTS), spread, strength
    9. the film: key, permille, e_min, e_max (kept >= e_min), rate, fallback; the usable previous exposure (10^u, u in -3..3); the
       curve, white, the table's kind and the gamma of a gamma table, dither
   10. the drivers: Temporal's sparse (none, 2, 3, the stride of 7), whether it filters, demodulate, the film's kind (none, Film(),
       the drawn one)

Every input of an image call is made on the device by code other campaigns pin (DeviceScene.guides, the masked render), copied to
the host and handed to the restatements; expected values come only from them and from the oracle (c.ob), never from a second run
of the code under test.  tests/test_fuzz_image.py pins the restatements on every seed of the pytest slice and judges what the slice
covers, without a GPU; tests/test_gpu_fuzz_image.py runs the slice.  Every comparison is on bits with NaN = NaN, RGB8 and masks
exactly.

    python tests/fuzz_image.py [seconds=240] [first_seed=0]

prints one line per mismatch with the seed that reproduces it, and a summary."""
import ctypes as C
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

import denoise_restatement as DNR  # noqa: E402
import film_restatement as FR  # noqa: E402
import fuzz_features as FF  # noqa: E402
import fuzz_gpu as F  # noqa: E402
import glare_restatement as GR  # noqa: E402
import upsample_restatement as UR  # noqa: E402
from bitcmp import same  # noqa: E402
from fuzz_lens import camera_numbers, camera_of, differ, guides, product_camera, sigma_p  # noqa: E402
from guarded_alloc import GUARD, guarded, untouched  # noqa: E402

sqt = FF.sqt
dn = importlib.import_module("squigly-trace_amd.denoise")
fm = importlib.import_module("squigly-trace_amd.film")
f32 = np.float32
N = 400
SLICE = range(1000, 1000 + N)                 # the pytest slice: tests/test_fuzz_image.py judges it, tests/test_gpu_fuzz_image.py runs it
BIG_SIDES = (17, 31, 33, 48, 65, 70)          # one under and one over a 16-tile, past a 64-lane row segment, pyramid levels >= 5
PIXEL_CAP = 2400                              # the oracle's first-hit walk of three cameras stays affordable without a GPU
CAMERAS = ("first", "second", "close")
PASS_WEIGHTS = np.array([1, 1, 2, 2, 2, 3, 4, 5]) / 20          # of passes 1..8: the largest step is 2^(passes - 1)
SIGMA_LS, EPS_LS, SIGMA_SCALES, COS_NS = (0.5, 4.0, 1e30, 1e-30), (0.0, 1e-3, 1.0), (1.0, 50.0, np.inf), (0.9, 0.0, -1.0)
GAINS, GAIN_WEIGHTS = (0.0, 0.6, 1.0, 1.5, 1e30, -0.75), np.array([2, 5, 5, 4, 2, 2]) / 20
THRESHOLDS, CEILINGS, SPREADS, STRENGTHS = (0.0, 0.25, 1.0, 1e30), (None, 4.0, 16.0, 3e38), (0.0, 0.5, 1.0, 2.0), (0.0, 0.1, 1.0, 1e30)
LEVEL_WEIGHTS = np.array([8, 8, 10, 10, 10, 12, 12, 12, 18]) / 100          # of levels 0..8
KEYS, PERMILLES, E_MINS, E_MAXS = (0.18, 1e-3, 100.0, 0.5), (1, 500, 900, 1000), (2.0 ** -10, 1e-38, 1.0, 0.25), (None, 2.0 ** 10, 3e38, 4.0)
RATES, FALLBACKS, WHITES, LUTS = (0.0, 0.5, 1.0), (1.0, 1e-30, 3e38, 0.25), (np.inf, 4.0, 1e-3), (None, "srgb", "gamma")
SENT = {"sum": 5.5, "sum2": -6.5, "count": 77, "avg": 8.25, "rgb": 99}       # fuzz_features' sentinels of a masked call
PERIOD = 2                                    # of the Temporal: the third frame takes the first's sample range again
WORK_GUARD = 4096                             # bytes behind the filter's workspace that must stay as they were
GUIDE_FIELDS = ("tri", "point", "normal", "surf", "emit")


def edge_pixels(tri):
    """How many pixels have a hit and a 4-neighbour without one."""
    hit = tri >= 0
    miss, near = ~hit, np.zeros_like(hit)
    near[1:] |= miss[:-1]
    near[:-1] |= miss[1:]
    near[:, 1:] |= miss[:, :-1]
    near[:, :-1] |= miss[:, 1:]
    return int((hit & near).sum())


def case(seed):
    c = FF.case(seed)
    rng = np.random.default_rng([seed, 4])
    # 1. the image
    c.case_w, c.case_h = c.w, c.h
    own, big = rng.random(2) < 0.5, rng.choice(BIG_SIDES, 2)
    rows, cols = (c.w if own[0] else int(big[0])), (c.h if own[1] else int(big[1]))
    if rows * cols > PIXEL_CAP:
        if rows >= cols:
            rows = c.w
        else:
            cols = c.h
    c.w, c.h, c.shard, c.rows = rows, cols, FF.WHOLE, list(range(rows))
    # 2. the cameras
    p0, a0 = camera_numbers(c.camt)
    step = rng.normal(0, 1, 6)
    p1 = tuple(float(f32(p + 0.1 * c.scale * s)) for p, s in zip(p0, step[:3]))
    a1 = tuple(float(f32(a + 0.1 * s)) for a, s in zip(a0, step[3:]))
    c.motion = (p0, a0, p1, a1)                                         # camera_of(c, "close") is its pose at 1
    c.edges = {name: edge_pixels(guides(c, name)["tri"]) for name in CAMERAS}
    c.cam_name = max(CAMERAS, key=lambda name: (c.edges[name], -CAMERAS.index(name)))
    c.previous = tuple(name for name in CAMERAS if name != c.cam_name)
    # 3. the guide poison
    c.poisoned = bool(rng.random() < 0.25)
    n_poison, at, kinds, comps = int(rng.integers(2, 7)), rng.random(6), rng.integers(0, 4, 6), rng.integers(0, 3, 6)
    hit = np.flatnonzero(guides(c, c.cam_name)["tri"].reshape(-1) >= 0)
    among = hit if len(hit) else np.arange(rows * cols)
    c.poison = [(int(among[int(u * len(among))]), int(k), int(m)) for u, k, m in zip(at[:n_poison], kinds, comps)] if c.poisoned else []
    # 4. the masked render
    c.ispp = int(rng.integers(1, 5))
    u, j = rng.random(), int(rng.integers(1, max(2, c.ispp)))
    c.split = None if c.ispp < 2 else 1 if u < 0.5 else j
    c.live_kind = np.digitize(rng.random((rows, cols)), [0.2, 0.5]).astype(np.int8)          # 0 neither, 1 the first range, 2 both
    # 5. the scale of the colour
    c.k = int(rng.integers(-24, 25))
    # 6. the filter
    c.passes = int(rng.choice(np.arange(1, 9), p=PASS_WEIGHTS))
    c.sigma_l, c.eps_l = float(rng.choice(SIGMA_LS)), float(rng.choice(EPS_LS))
    c.sigma_scale, c.squarings = float(rng.choice(SIGMA_SCALES)), int(rng.integers(0, 9))
    # 7. the sparse frame
    c.stride = int(rng.integers(1, 17))
    c.offset = tuple(int(v) for v in rng.integers(0, c.stride, 2))
    c.cos_n, c.sparse_scale = float(rng.choice(COS_NS)), float(rng.choice(SIGMA_SCALES))
    # 8. the glare
    c.e_kind, c.exposure = int(rng.integers(0, 2)), float(f32(10.0 ** rng.uniform(-2, 2)))
    c.gain = tuple(float(v) for v in rng.choice(GAINS, 3, p=GAIN_WEIGHTS))
    c.threshold = float(rng.choice(THRESHOLDS))
    above = float(np.nextafter(f32(c.threshold), f32(np.inf)))
    ceiling = CEILINGS[int(rng.integers(0, 4))]
    c.ceiling = above if ceiling is None or not f32(ceiling) > f32(c.threshold) else ceiling
    c.levels = int(rng.choice(np.arange(9), p=LEVEL_WEIGHTS))
    c.spread, c.strength = float(rng.choice(SPREADS)), float(rng.choice(STRENGTHS))
    # 9. the film
    e_min, e_max = float(rng.choice(E_MINS)), E_MAXS[int(rng.integers(0, 4))]
    c.meter = dict(key=float(rng.choice(KEYS)), permille=int(rng.choice(PERMILLES)), e_min=e_min,
                   e_max=e_min if e_max is None or e_max < e_min else e_max, rate=float(rng.choice(RATES)), fallback=float(rng.choice(FALLBACKS)))
    c.prev_usable = float(f32(10.0 ** rng.uniform(-3, 3)))
    c.curve, c.white = FR.CURVES[int(rng.integers(0, 5))], float(rng.choice(WHITES))
    c.lut_kind, c.gamma, c.dither = LUTS[int(rng.integers(0, 3))], float(rng.choice([1.0, 2.2, 0.45])), bool(rng.random() < 0.5)
    # 10. the drivers
    c.t_sparse = (None, 2, 3, c.stride)[int(rng.integers(0, 4))]
    c.t_denoise, c.demodulate = bool(rng.random() < 0.5), bool(rng.random() < 0.5)
    c.film_kind = ("none", "plain", "drawn")[int(rng.integers(0, 3))]
    return c


# ---- what the case stands for ------------------------------------------------------------------------------------------------
def filter_params(c):
    return dict(passes=c.passes, sigma_l=c.sigma_l, eps_l=c.eps_l, sigma_p=sigma_p(c, c.sigma_scale), normal_squarings=c.squarings)


def sparse_stops(c):
    return dict(sigma_p=sigma_p(c, c.sparse_scale), cos_n=c.cos_n)


def glare_params(c):
    return dict(threshold=c.threshold, ceiling=c.ceiling, levels=c.levels, spread=c.spread, strength=c.strength)


def lut_of(c):
    """The table of the case, a host array: None, srgb_lut(256) or gamma_lut(g, 2)."""
    return {None: lambda: None, "srgb": lambda: fm.srgb_lut(256), "gamma": lambda: fm.gamma_lut(c.gamma, 2)}[c.lut_kind]()


def film_spec(c, curve=None):
    """develop's keyword arguments under `curve` (default: the case's): the reference curve takes neither a table nor dither."""
    curve = c.curve if curve is None else curve
    if curve == "reference":
        return dict(curve=curve)
    return dict(curve=curve, white=c.white, lut=lut_of(c), dither=c.dither)


def poisoned(c, g):
    """A copy of the host guides g (a dict of arrays) with the case's poison."""
    g = {k: v.copy() for k, v in g.items()}
    for at, kind, m in c.poison:
        y, x = divmod(at, c.h)
        if kind == 0:
            g["normal"][y, x, m] = np.nan
        elif kind == 1:
            g["normal"][y, x] = 0
        elif kind == 2:
            g["point"][y, x, m] = np.inf
        else:
            g["tri"][y, x] = -1
    return g


def want_counts(c):
    """The counts the masked render leaves: 0, the split and spp."""
    return np.where(c.live_kind == 0, 0, np.where(c.live_kind == 1, c.ispp if c.split is None else c.split, c.ispp)).astype(np.int32)


def oracle_frame(c, name=None):
    """(avg, rgb8) of the oracle's dense frame of c.ispp samples under a camera of the case (default: the chosen one)."""
    name = c.cam_name if name is None else name
    store = c.__dict__.setdefault("_frames", {})
    if name not in store:
        store[name] = c.ob.render(camera_of(c, name), c.ispp, c.w, c.h)[:2]
    return store[name]


def scaled(c, avg):
    with np.errstate(all="ignore"):
        return (np.asarray(avg, f32) * f32(2.0 ** c.k)).astype(f32)


def demodulated(g, avg, var):
    """denoise.demodulated in numpy: (x, var, ok, scale), each step one float32 operation."""
    surf, emit = g["surf"], g["emit"]
    ok = ((g["tri"] >= 0) & (surf > 0).all(-1))[..., None]
    with np.errstate(all="ignore"):
        x = np.where(ok, (avg - emit) / np.where(ok, surf, f32(1)), avg).astype(f32)
        ls = (f32(0.25) * surf[..., 0] + f32(0.5) * surf[..., 1]) + f32(0.25) * surf[..., 2]
        scale = np.where(ok[..., 0], ls * ls, f32(1)).astype(f32)
        return x, None if var is None else (var / scale).astype(f32), ok, scale


def remodulated(g, out, out_var, ok, scale):
    with np.errstate(all="ignore"):
        return np.where(ok, out * g["surf"] + g["emit"], out).astype(f32), None if out_var is None else (out_var * scale).astype(f32)


# ---- one case on the GPU -----------------------------------------------------------------------------------------------------
def run_case(seed):
    """Every check of the seed; returns the list of mismatch messages (empty: all equal).  A refusal is a mismatch."""
    import torch
    F.load_libraries()
    tp = importlib.import_module("squigly-trace_amd.temporal")
    if FF.DEVICE_ERROR:
        raise RuntimeError(f"not run: the device reported an error earlier in this process ({FF.DEVICE_ERROR[0]})")
    c = case(seed)
    bad = []
    w, h, spp = c.w, c.h, c.ispp
    dev = "cuda:0"
    i32 = torch.int32
    cams = {"first": sqt.camera_from_text(c.camt), "second": sqt.camera_from_text(c.camt2), "close": product_camera(camera_of(c, "close"))}
    cam = cams[c.cam_name]
    ds = sqt.DeviceScene(FF.product_bih(c), 0)

    def host(t):
        return t.cpu().numpy()

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def zeros(*shape, dtype=torch.float32):
        return torch.zeros(shape, dtype=dtype, device=dev)

    def bits_equal(a, b):
        return a is b is None or torch.equal(a.view(i32), b.view(i32))

    def check(what, got, want):
        """got, want: arrays or tuples of them (None = absent); float32 on bits with NaN = NaN, everything else exactly."""
        got, want = (got if isinstance(got, (tuple, list)) else (got,)), (want if isinstance(want, (tuple, list)) else (want,))
        for i, (g, e) in enumerate(zip(got, want)):
            if (g is None) != (e is None):
                bad.append(f"{what}: result {i} is {'absent' if g is None else 'present'}")
                return False
            if g is None:
                continue
            g = host(g) if isinstance(g, torch.Tensor) else np.asarray(g)
            e = np.asarray(e)
            if g.shape != e.shape:
                bad.append(f"{what}: result {i} has shape {g.shape}, {e.shape} expected")
                return False
            if not (same(g, e) if e.dtype == f32 else np.array_equal(g, e)):
                n = differ(g, e) if e.dtype == f32 and e.ndim == 3 else int((g != e).sum())
                bad.append(f"{what}: result {i} differs from the restatement ({n} of {e.size // (3 if e.ndim == 3 else 1)})")
                return False
        return True

    try:
        for k, val in c.knobs.items():
            ds.set_option(k, val)
        ds.set_option("slots", c.slots)
        ds.set_option("deep", c.deep)
        # ---- the inputs: the guides (and their poisoned copy) and a masked render over two ranges
        g_dev = ds.guides(cam, w, h)
        torch.cuda.synchronize()
        g_clean = {f: host(getattr(g_dev, f)) for f in GUIDE_FIELDS}
        G = poisoned(c, g_clean)
        gp = dn.Guides(*(up(G[f]) for f in GUIDE_FIELDS)) if c.poisoned else g_dev
        tri, nrm, pnt = G["tri"], G["normal"], G["point"]
        sums, sums2, avg, counts = zeros(w, h, 3), zeros(w, h, 3), zeros(w, h, 3), zeros(w, h, dtype=i32)
        in_first, in_both = up((c.live_kind >= 1).astype(np.uint8)), up((c.live_kind == 2).astype(np.uint8))
        for k0, k1, m in ([(0, spp, in_first)] if c.split is None else [(0, c.split, in_first), (c.split, spp, in_both)]):
            ds.render_rows_masked(cam, spp, w, h, k0, k1, sums, mask=m, sums2=sums2, counts=counts, out_avg=avg, want_rgb=False)
        torch.cuda.synchronize()
        S, Q, A, NC = host(sums), host(sums2), host(avg), host(counts)
        dense_avg, dense_rgb = oracle_frame(c)
        full = NC == spp
        if not np.array_equal(NC, want_counts(c)) or not same(A[full], dense_avg[full]):
            bad.append("the masked render of the inputs: the counts, or the average of a fully sampled pixel, are not the oracle's")
        # ---- 1. the variance
        var = dn.denoise_variance(sums, sums2, counts)
        check("denoise_variance", var, DNR.variance(S, Q, NC))
        V = host(var)
        # ---- 2. the filter: with and without var in forms 0, 1, 2; in place; a NaN workspace of exactly workspace_bytes
        P = filter_params(c)
        want_v = DNR.denoise(A, tri, nrm, pnt, var=V, **P)
        want_n = DNR.denoise(A, tri, nrm, pnt, var=None, **P)
        for v, want in ((var, want_v), (None, want_n)):
            outs = [dn.denoise(avg, gp.tri, gp.normal, gp.point, var=v, form=form, **P) for form in (0, 1, 2)]
            for form, got in enumerate(outs):
                check(f"denoise {P}, {'with' if v is not None else 'without'} var, form {form}", got, want)
            if not all(bits_equal(a, b) for o in outs[1:] for a, b in zip(outs[0], o)):
                bad.append(f"denoise {P}, {'with' if v is not None else 'without'} var: forms 0, 1 and 2 differ from each other")
        col, cv = avg.clone(), var.clone()
        check(f"denoise {P}, in place", dn.denoise(col, gp.tri, gp.normal, gp.point, var=cv, out=(col, cv), **P), want_v)
        need = dn.workspace_bytes(w, h)
        work = torch.full((need + WORK_GUARD,), 0xFF, dtype=torch.uint8, device=dev)
        out, out_v = torch.empty_like(avg), torch.empty_like(var)
        par = dn.make_params(**P)
        dn.check(dn.lib().sq_denoise_device(0, w, h, avg.data_ptr(), var.data_ptr(), gp.tri.data_ptr(), gp.normal.data_ptr(),
                                            gp.point.data_ptr(), C.byref(par), out.data_ptr(), out_v.data_ptr(), work.data_ptr(), need, None))
        torch.cuda.synchronize()
        check(f"denoise {P}, a NaN workspace of {need} bytes", (out, out_v), want_v)
        if not bool((work[need:] == 0xFF).all()):
            bad.append(f"denoise {P}: the bytes behind the workspace's {need} were written")
        # ---- 3. the sparse frame
        s, (oy, ox), stops = c.stride, c.offset, sparse_stops(c)
        what = f"stride {s} offset {c.offset} {stops}"
        mask = dn.sparse_mask(gp, s, c.offset, **stops)
        want_mask = UR.sparse_mask(tri, nrm, pnt, s, oy, ox, **stops)
        check(f"sparse_mask, {what}", mask, want_mask)
        B = {"sum": torch.full((w, h, 3), SENT["sum"], dtype=torch.float32, device=dev),
             "sum2": torch.full((w, h, 3), SENT["sum2"], dtype=torch.float32, device=dev),
             "count": torch.full((w, h), SENT["count"], dtype=i32, device=dev),
             "avg": torch.full((w, h, 3), SENT["avg"], dtype=torch.float32, device=dev),
             "rgb": torch.full((w, h, 3), SENT["rgb"], dtype=torch.uint8, device=dev)}
        ds.render_rows_masked(cam, spp, w, h, 0, spp, B["sum"], mask=mask, sums2=B["sum2"], counts=B["count"], out_avg=B["avg"], out_rgb=B["rgb"])
        torch.cuda.synchronize()
        M = host(mask)
        got = {k: host(t) for k, t in B.items()}
        on, off = M != 0, M == 0
        if not (same(got["avg"][on], dense_avg[on]) and np.array_equal(got["rgb"][on], dense_rgb[on]) and (got["count"][on] == spp).all()):
            bad.append(f"render_rows_masked under the sparse mask, {what}: a set pixel differs from the oracle's dense frame")
        if not all((got[k][off] == SENT[k]).all() for k in SENT):
            bad.append(f"render_rows_masked under the sparse mask, {what}: a clear pixel lost a sentinel")
        for v, hv in ((var, V), (None, None)):
            check(f"upsample, {what}, {'with' if v is not None else 'without'} var", dn.upsample(B["avg"], gp, mask, s, c.offset, var=v, **stops),
                  UR.upsample(got["avg"], tri, nrm, pnt, M, s, oy, ox, var=hv, **stops))
        M2 = (M | (c.live_kind >= 1)).astype(np.uint8)
        check(f"upsample, {what}, under a caller's mask", dn.upsample(B["avg"], gp, up(M2), s, c.offset, var=var, **stops),
              UR.upsample(got["avg"], tri, nrm, pnt, M2, s, oy, ox, var=V, **stops))
        # ---- 4. the glare: forms 1, 2, 0 with the colour at its allocation and one float into it; in place
        X = scaled(c, A)
        settings = dict(gain=c.gain, threshold=c.threshold, ceiling=c.ceiling, spread=c.spread, strength=c.strength)
        e_dev = up(np.array([c.exposure], f32))
        want = GR.glare(X, c.exposure, levels=c.levels, **settings)
        need = dn.glare_work_bytes(w, h, c.levels)
        if need != GR.work_bytes(w, h, c.levels):
            bad.append(f"glare_work_bytes({w}, {h}, {c.levels}) = {need}, {GR.work_bytes(w, h, c.levels)} expected")

        def glare_run(skip, form, exposure, in_place=False):
            src, src_whole = guarded(torch, X.shape, skip, -555.0)
            src.copy_(torch.from_numpy(X))
            out, out_whole = (src, src_whole) if in_place else guarded(torch, X.shape, skip, -777.0)
            work_whole = torch.full((need // 4 + GUARD,), float("nan"), dtype=torch.float32, device=dev)
            got = dn.glare(src, exposure=exposure, levels=c.levels, form=form, out=out, work=work_whole.view(torch.uint8)[:need] if need else None,
                           **settings)
            torch.cuda.synchronize()
            if not (untouched(out_whole, skip, X.size, -555.0 if in_place else -777.0) and untouched(work_whole, 0, need // 4, float("nan"))):
                bad.append(f"glare {settings} levels {c.levels}, form {form}, skip {skip}: a guard around d_out or behind the workspace was written")
            if not in_place and not same(host(src), X):
                bad.append(f"glare {settings} levels {c.levels}, form {form}, skip {skip}: d_color was written")
            return host(got)

        results = []
        for form in (1, 2, 0):
            for skip in (0, 1):
                got = glare_run(skip, form, e_dev if (form + skip + c.e_kind) % 2 else c.exposure)
                results.append(got)
                check(f"glare {settings} levels {c.levels} exposure {c.exposure}, form {form}, skip {skip}", got, want)
        if not all(same(r, results[0]) for r in results[1:]):
            bad.append(f"glare {settings} levels {c.levels}: the forms and alignments differ from each other")
        check(f"glare {settings} levels {c.levels}, in place", glare_run(c.e_kind, 0, e_dev if c.e_kind else c.exposure, in_place=True), want)
        # ---- 5. the film: histogram, expose under the drawn meter and every kind of previous exposure, develop under every curve
        x_dev = up(X)
        hist = fm.histogram(x_dev)
        Hh = FR.histogram(X)
        check("film.histogram", host(hist).astype(np.int64), Hh)
        for prev in (None, c.prev_usable, 0.0, np.nan, np.inf):
            got = fm.expose(hist, prev=None if prev is None else up(np.array([prev], f32)), **c.meter)
            check(f"film.expose {c.meter}, prev {prev}", got, np.array([FR.expose(Hh, prev, **c.meter)], f32))
        e_want = FR.expose(Hh, None, **c.meter)
        e_film = fm.expose(hist, **c.meter)
        for ci, curve in enumerate(FR.CURVES):
            spec = film_spec(c, curve)
            lut = spec.get("lut")
            spec_dev = dict(spec, lut=None if lut is None else up(lut)) if "lut" in spec else spec
            want = FR.develop(O, X, e_want, **spec)
            for skip in (0, 1):
                src, _ = guarded(torch, X.shape, skip, -555.0)
                src.copy_(torch.from_numpy(X))
                got = fm.develop(src, exposure=e_film if (ci + skip) % 2 else float(e_want), want_display=True, **spec_dev)
                check(f"film.develop {spec}, exposure {e_want}, skip {skip}", got, want)
        # ---- 6. the drivers over the three cameras as a sequence: the previous two, then the chosen one
        sp = sigma_p(c)
        tparams = dict(alpha_min=0.1, max_history=32, cos_n=0.9, sigma_p=sp)
        dparams = dict(filter_params(c)) if c.t_denoise else None

        def make_film():
            if c.film_kind == "none":
                return None
            if c.film_kind == "plain":
                return sqt.Film()
            return sqt.Film(auto=c.meter, glare=sqt.Glare(**glare_params(c)), balance=c.gain, **film_spec(c))

        def demod(g, x, v):
            ok = ((g.tri >= 0) & (g.surf > 0).all(-1))[..., None]
            x = torch.where(ok, (x - g.emit) / torch.where(ok, g.surf, torch.ones_like(g.surf)), x)
            ls = (0.25 * g.surf[..., 0] + 0.5 * g.surf[..., 1]) + 0.25 * g.surf[..., 2]
            scale = torch.where(ok[..., 0], ls * ls, torch.ones_like(ls))
            return x, None if v is None else v / scale, ok, scale

        def remod(g, out, out_v, ok, scale):
            return torch.where(ok, out * g.surf + g.emit, out), None if out_v is None else out_v * scale

        film = make_film()
        t = tp.Temporal(ds, w, h, spp, period=PERIOD, denoise=dparams, demodulate=c.demodulate, sigma_p=sp, film=film, sparse=c.t_sparse)
        blocks = [tp.history(w, h, 0), tp.history(w, h, 0)]
        full_counts = torch.full((w, h), spp, dtype=i32, device=dev)
        prev, prev_cam, avgs, images = None, None, [], []
        for f, name in enumerate(c.previous + (c.cam_name,)):
            cm = cams[name]
            what = f"Temporal(sparse={c.t_sparse}, denoise={dparams}, demodulate={c.demodulate}, film {c.film_kind}) frame {f} ({name} camera)"
            r = t.step(cm)
            g = ds.guides(cm, w, h)
            live, lattice = None, None
            if c.t_sparse is not None:
                lattice = dict(stride=c.t_sparse, offset=UR.lattice_offset(f, c.t_sparse), sigma_p=sp, cos_n=0.9)
                live = dn.sparse_mask(g, **lattice)
            s1, s2 = zeros(w, h, 3), zeros(w, h, 3)
            k0 = (f % PERIOD) * spp
            ds.render_rows_masked(cm, spp * PERIOD, w, h, k0, k0 + spp, s1, mask=live, sums2=s2, want_avg=False, want_rgb=False)
            noisy = s1 / float(spp)
            x, v = noisy, dn.denoise_variance(s1, s2, full_counts)
            if c.demodulate:
                x, v, ok, scale = demod(g, x, v)
            if live is not None:
                x, v = dn.upsample(x, g, live, var=v, **lattice)
            o, ov, length = tp.accumulate(x, v, g, prev_cam, prev, blocks[f & 1], alpha=tp.frame_alpha(ds, g.tri), **tparams)
            if dparams is not None:
                o, ov = dn.denoise(o, g.tri, g.normal, g.point, var=ov, **dparams)
            if c.demodulate:
                o, ov = remod(g, o, ov, ok, scale)
            torch.cuda.synchronize()
            if not (bits_equal(r[0], o) and bits_equal(r[1], ov) and torch.equal(r[2], length) and bits_equal(t.noisy, noisy)
                    and torch.equal(t.history, blocks[f & 1])):
                bad.append(f"{what}: avg, var, length, noisy or the history differs from the primitive calls")
            if (t.live is None) != (live is None) or (live is not None and not torch.equal(t.live, live)):
                bad.append(f"{what}: live differs from sparse_mask at lattice_offset")
            if film is None and not torch.equal(r[3], tp.tonemap(o)):
                bad.append(f"{what}: rgb differs from tonemap(avg)")
            avgs.append(host(r[0]))
            images.append(host(r[3]))
            prev, prev_cam = blocks[f & 1], cm
        if film is not None:
            drawn = c.film_kind == "drawn"
            want = GR.chain(O, avgs, film_spec(c) if drawn else {}, c.meter if drawn else None, glare_params(c) if drawn else None,
                            c.gain if drawn else None)
            for f in range(3):
                if not np.array_equal(images[f], want[f][0]):
                    bad.append(f"Temporal film {c.film_kind} {film_spec(c)} {c.meter} {glare_params(c)} balance {c.gain}: frame {f}'s rgb differs "
                               f"from glare_restatement.chain in {int((images[f] != want[f][0]).any(-1).sum())} pixels")
            # (Film.exposure_state reads a state that is not finite and > 0 as None: with rate 1 and t far below p, p + (t - p) is 0)
            state = float(want[2][1]) if FR.usable(want[2][1]) else None
            if drawn and film.exposure_state != state:
                bad.append(f"Temporal film: the exposure state is {film.exposure_state}, {state} expected")
        # denoise_frame on the chosen camera's frame: the restatement with the demodulation restated in numpy
        got = dn.denoise_frame(ds, cam, w, h, avg, var=var, demodulate=c.demodulate, **P)
        if c.demodulate:
            x, v, ok, scale = demodulated(g_clean, A, V)
            want = remodulated(g_clean, *DNR.denoise(x, g_clean["tri"], g_clean["normal"], g_clean["point"], var=v, **P), ok, scale)
        else:
            want = DNR.denoise(A, g_clean["tri"], g_clean["normal"], g_clean["point"], var=V, **P)
        check(f"denoise_frame(demodulate={c.demodulate}) {P}", got, want)
        # render_sparse: its own resident scene, against the chain made by hand on this one
        film, film2 = make_film(), make_film()
        got = sqt.render_sparse(FF.product_bih(c), cam, spp, (w, h), s, c.offset, denoise=dparams, film=film, sigma_p=stops["sigma_p"],
                                cos_n=c.cos_n, demodulate=c.demodulate)
        g = ds.guides(cam, w, h)
        live = dn.sparse_mask(g, s, c.offset, **stops)
        s1, s2 = zeros(w, h, 3), (zeros(w, h, 3) if dparams is not None else None)
        a, _ = ds.render_rows_masked(cam, spp, w, h, 0, spp, s1, mask=live, sums2=s2, want_rgb=False)
        x, v = a, (dn.denoise_variance(s1, s2, full_counts) if dparams is not None else None)
        if c.demodulate:
            x, v, ok, scale = demod(g, x, v)
        o, ov = dn.upsample(x, g, live, s, c.offset, var=v, **stops)
        if dparams is not None:
            o, ov = dn.denoise(o, g.tri, g.normal, g.point, var=ov, **dparams)
        if c.demodulate:
            o, _ = remod(g, o, ov, ok, scale)
        torch.cuda.synchronize()
        want = host(film2(o)) if film2 is not None else sqt.debug_eval("tonemap", host(o).reshape(-1, 3), device=0).reshape(w, h, 3)
        if not np.array_equal(got, want):
            bad.append(f"render_sparse(stride {s}, offset {c.offset}, denoise={dparams}, film {c.film_kind}, demodulate={c.demodulate}) differs "
                       "from the chain made by hand")
    except sqt.SquiglyError as e:
        if " failed: " in str(e):                                       # a HIP error is no refusal: nothing more runs on this device
            FF.DEVICE_ERROR.append(f"seed {seed}: {e}")
            raise
        bad.append(f"refused: {e}")
    except ValueError as e:                                             # a driver's refusal of its arguments
        bad.append(f"refused: {e}")
    except RuntimeError as e:                                           # torch's own report of a HIP error (a synchronize, a copy)
        if "HIP error" in str(e) or "CUDA error" in str(e):
            FF.DEVICE_ERROR.append(f"seed {seed}: {e}")
        raise
    finally:
        ds.close()
    return bad


def describe(c):
    return (f"seed {c.seed}: {len(c.v)} tris, {c.w}x{c.h} (the case's {c.case_w}x{c.case_h}), camera {c.cam_name} (edge pixels {c.edges}), "
            f"poison {c.poison}, spp {c.ispp} split {c.split}, live kinds {np.bincount(c.live_kind.reshape(-1), minlength=3).tolist()}, "
            f"k {c.k}, filter passes {c.passes} sigma_l {c.sigma_l} eps_l {c.eps_l} sigma_p x{c.sigma_scale} squarings {c.squarings}, "
            f"sparse stride {c.stride} offset {c.offset} cos_n {c.cos_n} sigma_p x{c.sparse_scale}, glare exposure {c.exposure} "
            f"({'device' if c.e_kind else 'number'}) gain {c.gain} {glare_params(c)}, meter {c.meter} prev {c.prev_usable}, curve {c.curve} "
            f"white {c.white} lut {c.lut_kind} gamma {c.gamma} dither {c.dither}, Temporal sparse {c.t_sparse} denoise {c.t_denoise} "
            f"demodulate {c.demodulate} film {c.film_kind}, {c.knobs}")


def main(budget=240.0, seed=0):
    return F.campaign("fuzz_image", run_case, budget, seed)


if __name__ == "__main__":
    sys.exit(main(float(sys.argv[1]) if len(sys.argv) > 1 else 240.0, int(sys.argv[2]) if len(sys.argv) > 2 else 0))
