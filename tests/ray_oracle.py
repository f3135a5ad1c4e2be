"""Caller-given rays: the families of rays the query tests trace, and what the CPU oracle says of any ray.

Belongs here: a generator of rays (far from the camera, on surfaces, axis-aligned, on split planes, non-finite, degenerate), the
oracle's answer for a ray batch (intersectBIH, Lib.raytrace, Lib.raycast) and the thin wrappers that bring a query's result to the
host.  The generators draw from default_rng(seed) in a fixed order: recorded expectations depend on it.

The oracle has no entry point for a caller-given ray.  Its raytrace is reached through sample_radiance with a camera that is not a
rotation: pos = o, rot = [dx, dy, dz, 0, 0, 0, 0, 0, 0] makes rotVert return d for every pixel, and with w = h = 1, y = 0,
samples = N, x = seed div N, k = seed mod N the generator is mkTFGen seed.  A -0.0 direction component would come out as +0.0
(-0 + 0), so the radiance families hold no negative-zero direction components (positive_zeros)."""
import ctypes as C

import numpy as np

from bitcmp import ibits, nan_eq

f32 = np.float32
N_FAMILY = 20000
FAMILIES = ("free", "surface", "axis", "degenerate")                   # of the intersection queries
RADIANCE_FAMILIES = ("free", "surface", "to_light", "degenerate")      # of the radiance queries
TRICK_SAMPLES = 1 << 30               # N of the trick camera: x = seed div N fits an int for |seed| < 2^60


# ---- ray families ----------------------------------------------------------------------------------------------------
def unit_dirs(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def family_free(rng, bounds, n):
    """Origins uniform in the root box grown by 20 %, directions uniform on the sphere with |d| log-uniform in [1e-3, 1e3]."""
    lo, hi = bounds[:3].astype(np.float64), bounds[3:].astype(np.float64)
    c, half = (lo + hi) / 2, (hi - lo) / 2 * 1.2
    o = c + rng.uniform(-1, 1, (n, 3)) * half
    d = unit_dirs(rng, n) * 10.0 ** rng.uniform(-3, 3, (n, 1))
    return o.astype(f32), d.astype(f32)


def family_surface(rng, tris, limits, n):
    """Barycentric points on random triangles; a third of the directions with |d|^2 inside the culling limits, the rest |d| in
    [1e-2, 1e2]."""
    t = tris[rng.integers(0, len(tris), n)]
    u, v = rng.uniform(0, 1, (2, n, 1)).astype(f32)
    flip = (u + v) > 1
    u, v = np.where(flip, 1 - u, u), np.where(flip, 1 - v, v)
    o = (t["v0"] + u * (t["v1"] - t["v0"]) + v * (t["v2"] - t["v0"])).astype(f32)
    _, d2min, d2max = limits
    inside = np.arange(n) % 3 == 0
    mag = np.where(inside[:, None], np.sqrt(rng.uniform(d2min * 1.001, d2max * 0.999, (n, 1))), 10.0 ** rng.uniform(-2, 2, (n, 1)))
    return o, (unit_dirs(rng, n) * mag).astype(f32)


def family_axis(rng, bounds, nodes, n):
    """Directions along an axis (with signed zeros) and general ones; origins exactly on lmax / rmin planes of the tree's branches and
    on the faces of the root box."""
    lo, hi = bounds[:3], bounds[3:]
    o = (lo + rng.uniform(-0.1, 1.1, (n, 3)).astype(f32) * (hi - lo)).astype(f32)
    br = np.nonzero((nodes["kind"] & 3) != 3)[0]
    pick = br[rng.integers(0, len(br), n)]
    ax = nodes["kind"][pick] & 3
    plane = np.where(rng.integers(0, 2, n) == 1, nodes["lmax"][pick], nodes["rmin"][pick]).astype(f32)
    face = np.arange(n) % 4 == 3                              # a quarter on the root box's faces
    fax = rng.integers(0, 3, n)
    fval = np.where(rng.integers(0, 2, n) == 1, hi[fax], lo[fax]).astype(f32)
    ax = np.where(face, fax, ax)
    o[np.arange(n), ax] = np.where(face, fval, plane)
    d = np.zeros((n, 3), f32)
    k = rng.integers(0, 3, n)
    mag = (10.0 ** rng.uniform(-1, 1, n)).astype(f32)
    d[np.arange(n), k] = np.where(rng.integers(0, 2, n) == 1, mag, -mag)
    zeros = np.where(rng.integers(0, 2, (n, 3)) == 1, f32(-0.0), f32(0.0))
    d = np.where(d == 0, zeros, d)
    general = np.arange(n) % 5 == 4                           # some rays leave the plane obliquely
    d[general] = (unit_dirs(rng, int(general.sum())) * 1.1).astype(f32)
    return o, d


def family_degenerate(rng, bounds, n):
    """d = 0, NaN or +-inf components in o or d, |o| ~ 1e30, |d| ~ 1e-30 and 1e30, mixed with ordinary rays."""
    o, d = family_free(rng, bounds, n)
    kind = np.arange(n) % 8
    r = np.arange(n)
    comp = rng.integers(0, 3, n)
    specials = np.array([np.nan, np.inf, -np.inf], f32)[rng.integers(0, 3, n)]
    zsign = np.where(rng.integers(0, 2, (n, 3)) == 1, f32(-0.0), f32(0.0))
    d = np.where((kind == 0)[:, None], zsign, d)
    o[r[kind == 1], comp[kind == 1]] = specials[kind == 1]
    d[r[kind == 2], comp[kind == 2]] = specials[kind == 2]
    o[kind == 3] = (unit_dirs(rng, int((kind == 3).sum())) * 1e30).astype(f32)
    d[kind == 3] = -o[kind == 3] / f32(1e30)
    d[kind == 4] = (unit_dirs(rng, int((kind == 4).sum())) * 1e-30).astype(f32)
    d[kind == 5] = (unit_dirs(rng, int((kind == 5).sum())) * 1e30).astype(f32)
    d[r[kind == 6], comp[kind == 6]] = np.float32(0.0)        # one zero component: an inf in 1/d
    return o.astype(f32), d.astype(f32)


def family_to_light(rng, bounds, otris, n):
    """Origins uniform inside the root box; direction = (a random point on a random emissive triangle - origin) * 10^U(-1, 1)."""
    lo, hi = bounds[:3].astype(np.float64), bounds[3:].astype(np.float64)
    o = (lo + rng.uniform(0, 1, (n, 3)) * (hi - lo)).astype(f32)
    em = np.nonzero((otris["emit"] != 0).any(-1))[0]
    t = otris[em[rng.integers(0, len(em), n)]]
    u, v = rng.uniform(0, 1, (2, n, 1))
    flip = (u + v) > 1
    u, v = np.where(flip, 1 - u, u), np.where(flip, 1 - v, v)
    p = t["a"] + u * (t["b"] - t["a"]) + v * (t["c"] - t["a"])
    d = (p - o) * 10.0 ** rng.uniform(-1, 1, (n, 1))
    return o, d.astype(f32)


def positive_zeros(d):
    return np.where(d == 0, f32(0.0), d).astype(f32)               # -0.0 == 0: becomes +0.0


def make_families(bih, seed):
    """{family: (origins, directions)} of the intersection queries, N_FAMILY rays each."""
    rng = np.random.default_rng(seed)
    b = bih.bounds
    _, limits = bih.cull_boxes()
    return {
        "free": family_free(rng, b, N_FAMILY),
        "surface": family_surface(rng, bih.tris, limits, N_FAMILY),
        "axis": family_axis(rng, b, bih.nodes, N_FAMILY),
        "degenerate": family_degenerate(rng, b, N_FAMILY),
    }


def make_radiance_families(bih, otris, seed):
    """({family: (origins, directions)}, {family: seeds}) of the radiance queries: no -0 direction components; seeds small, above
    2^40 and negative, by thirds."""
    rng = np.random.default_rng(seed)
    b = bih.bounds
    _, limits = bih.cull_boxes()
    fam = {
        "free": family_free(rng, b, N_FAMILY),
        "surface": family_surface(rng, bih.tris, limits, N_FAMILY),
        "to_light": family_to_light(rng, b, otris, N_FAMILY),
        "degenerate": family_degenerate(rng, b, N_FAMILY),
    }
    fam = {k: (np.ascontiguousarray(o, f32), positive_zeros(d)) for k, (o, d) in fam.items()}
    for k, (o, d) in fam.items():
        assert not (np.signbit(d) & (d == 0)).any(), k
    seeds = {}
    for k in RADIANCE_FAMILIES:
        s = np.empty(N_FAMILY, np.int64)
        third = np.arange(N_FAMILY) % 3
        s[third == 0] = rng.integers(0, 1 << 20, int((third == 0).sum()))
        s[third == 1] = rng.integers(1 << 40, 1 << 60, int((third == 1).sum()))
        s[third == 2] = -rng.integers(1, 1 << 60, int((third == 2).sum()))
        seeds[k] = s
    return fam, seeds


# ---- the oracle's answer for any ray -----------------------------------------------------------------------------------------
def oracle_hits(ob, o, d):
    """(tri, dist, point) of the oracle's intersectBIH per ray; tri = -1 for Nothing."""
    n = len(o)
    tri = np.full(n, -1, np.int64)
    dist = np.zeros(n, f32)
    pt = np.zeros((n, 3), f32)
    for i in range(n):
        h = ob.intersect(o[i], d[i])
        if h.hit:
            tri[i], dist[i], pt[i] = h.tri, h.dist, (h.point.x, h.point.y, h.point.z)
    return tri, dist, pt


def check_hits(got, want, what):
    """tri equal; on hits dist and point bit-equal (NaN = NaN); misses exactly tri -1, dist +inf, point +0."""
    tri, dist, pt = got
    etri, edist, ept = want
    bad = tri != etri
    assert not bad.any(), (what, "tri", int(bad.sum()), np.nonzero(bad)[0][:8])
    hit = etri >= 0
    assert nan_eq(dist[hit], edist[hit]).all(), (what, "dist", int((~nan_eq(dist[hit], edist[hit])).sum()))
    assert nan_eq(pt[hit], ept[hit]).all(), (what, "point", int((~nan_eq(pt[hit], ept[hit])).any(-1).sum()))
    assert (ibits(dist[~hit]) == ibits(np.float32(np.inf))).all(), (what, "miss dist")
    assert (ibits(pt[~hit]) == 0).all(), (what, "miss point")


def trick_camera(O, o, d):
    cam = O.Camera()
    cam.pos = O.V3(float(o[0]), float(o[1]), float(o[2]))
    for j in range(9):
        cam.rot[j] = float(d[j]) if j < 3 else 0.0
    return cam


def oracle_raytrace(O, ob, o, d, seeds, k=0):
    """raytrace (mkTFGen (seed_i + k)) scene (Ray o_i d_i) 0 per ray, float32 [n, 3]."""
    L = O.lib()
    out = np.zeros((len(o), 3), f32)
    buf = (C.c_float * 3)()
    for i in range(len(o)):
        x, kk = divmod(int(seeds[i]) + k, TRICK_SAMPLES)           # floor division: kk in [0, N) for negative seeds too
        L.sqo_sample_radiance(ob._h, C.byref(trick_camera(O, o[i], d[i])), TRICK_SAMPLES, 1, 1, 0, x, kk, O.TRIG_CRD, 0, buf)
        out[i] = buf[:]
    return out


def oracle_raycast(O, ob, o, d):
    """1 * (0 + raycast scene (Ray o_i d_i)) per ray: the oracle's one-sample cast render of the trick camera."""
    out = np.zeros((len(o), 3), f32)
    for i in range(len(o)):
        avg, _, _ = ob.render(trick_camera(O, o[i], d[i]), 1, 1, 1, cast=True, want_rgb=False)
        out[i] = avg[0, 0]
    return out


# ---- a query's result on the host ----------------------------------------------------------------------------------------
def query(ds, o, d, **kw):
    import torch
    h = ds.intersect(o, d, **kw)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in h)


def raytrace(ds, o, d, seeds, **kw):
    import torch
    r = ds.raytrace(o, d, seeds=seeds, **kw)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in r)


def cast_from_queries(ds, bih, cam, spp, w, h, shard):
    """src/Lib.hs:141-151 (raycast) and :85-88 (the sample fold) in numpy float32, from two intersect calls."""
    o, d = ds.camera_rays(cam, w, h, shard=shard)
    h0 = ds.intersect(o, d)
    p0 = h0.point
    light = np.array([0, 3, -1], f32)
    p0n = p0.cpu().numpy()
    sdir = (light - p0n).astype(f32)                          # light - p0: the shadow ray's direction
    h1 = ds.intersect(p0, sdir)
    tri0, tri1, dist1 = h0.tri.cpu().numpy(), h1.tri.cpu().numpy(), h1.dist.cpu().numpy()
    v = (p0n - light).astype(f32)
    dl = np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]).astype(f32)   # norm (p0 - light)
    with np.errstate(all="ignore"):
        lit = ~((tri1 >= 0) & ~(dist1 > dl))                  # maybe True (\pos -> dist pos > dl)
        surf = bih.materials["surf"][bih.tris["mat"][np.where(tri0 >= 0, tri0, 0)]].astype(f32)
        c = np.where(lit[..., None], (f32(2) / dl)[..., None] * surf, f32(0)).astype(f32)
    s = np.zeros_like(c)
    for _ in range(spp):
        s = (s + c).astype(f32)
    avg = (f32(1) / f32(spp)) * s
    return np.where((tri0 >= 0)[..., None], avg, f32(0)).astype(f32)
