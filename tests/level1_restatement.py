"""Level-1 culling (squigly-trace_amd/csrc/sq_pack_level1.h, build_level1; sq_device.hip, level1_culled) restated in numpy.

The tables come from the packer's window (sq_packed_array "level1"); the three conditions are evaluated as the kernel evaluates
them: mollerTrumbore and the slab test in float32, one rounding per operation (tests/test_cull.py), the half-plane test in
binary64 with the kernel's operation order.  randomVector and the generator words come from the oracle.
"""
import ctypes as C
import importlib

import numpy as np
import pyoracle as O
from kernel_restatements import mt_accepts, slab_passes

f32 = np.float32
EPS = f32(0.0001)
LEVEL1 = np.dtype({"names": ["on", "n_classes", "o2max", "d2min", "d2max", "class_val", "class_box", "em_lo", "em_hi", "em_rho", "em_add"],
                   "formats": ["<i4", "<i4", "<f4", "<f4", "<f4", ("<f4", 4), ("<f4", (4, 6)), ("<f8", 3), ("<f8", 3), "<f8", "<f8"],
                   "offsets": [0, 4, 8, 12, 16, 20, 36, 136, 160, 184, 192], "itemsize": 200})


def tables(sqt, holder):
    """(Level1Cull record, {scalar: value}) of holder.scene, through sq_scene_pack."""
    L, h = sqt.lib(), C.c_void_p()
    sqt._native.check(L.sq_scene_pack(C.byref(holder.scene), C.byref(h)))
    try:
        data, n = C.c_void_p(), C.c_size_t()
        assert L.sq_packed_array(h, b"level1", C.byref(data), C.byref(n)) == 0
        assert n.value == LEVEL1.itemsize, n.value
        rec = np.frombuffer(C.string_at(data, n.value), LEVEL1)[0]
        scalars = {}
        for name in ("level1_on", "level1_zero", "n_emitters", "nonneg_materials"):
            v = C.c_int64()
            assert L.sq_packed_scalar(h, name.encode(), C.byref(v)) == 0, name
            scalars[name] = v.value
        assert scalars["level1_on"] == rec["on"]
    finally:
        L.sq_packed_free(h)
    return rec, scalars


def unit_float(n):
    n = np.asarray(n, np.uint32)
    return (f32(0) + f32(1) * (n.astype(f32) / f32(4294967296.0))).astype(f32)


def random_vectors(n1, n2):
    L = O.lib()
    out = np.empty((len(n1), 3), f32)
    for i in range(len(n1)):
        v = L.sqo_random_vector(int(n1[i]), int(n2[i]), 0)
        out[i] = (v.x, v.y, v.z)
    return out


def dot32(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def halfplane_misses_box(p0, d1, nd, lo, hi, m):
    """The kernel's binary64 test: does { p0 + t d1 + s nd : t >= 0 } provably miss [lo - m, hi + m]?  m: per row."""
    p, d, n = p0.astype(np.float64), d1.astype(np.float64), nd.astype(np.float64)
    g = 0.5 * (lo + hi)[None, :] - p
    h = 0.5 * (hi - lo)[None, :] + m[:, None]
    scale = np.zeros(len(p))
    for k in range(3):
        scale = scale + (np.abs(g[:, k]) + h[:, k])
    tol = 1e-9 * scale
    N = np.stack([d[:, 1] * n[:, 2] - d[:, 2] * n[:, 1], d[:, 2] * n[:, 0] - d[:, 0] * n[:, 2], d[:, 0] * n[:, 1] - d[:, 1] * n[:, 0]], 1)
    dist = np.abs(N[:, 0] * g[:, 0] + N[:, 1] * g[:, 1] + N[:, 2] * g[:, 2])
    rad = np.abs(N[:, 0]) * h[:, 0] + np.abs(N[:, 1]) * h[:, 1] + np.abs(N[:, 2]) * h[:, 2]
    plane = dist > rad + tol
    with np.errstate(all="ignore"):
        f = (d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1] + d[:, 2] * n[:, 2]) / (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2])
        w = d - f[:, None] * n
        side = w[:, 0] * g[:, 0] + w[:, 1] * g[:, 1] + w[:, 2] * g[:, 2] + np.abs(w[:, 0]) * h[:, 0] + np.abs(w[:, 1]) * h[:, 1] + np.abs(w[:, 2]) * h[:, 2]
    return plane | (side < -tol)


def ray_in_limits(T, p0, d1):
    with np.errstate(all="ignore"):
        df = f32(1) / d1
        nodf = -p0 * df
    fin = np.isfinite(p0).all(1) & np.isfinite(d1).all(1) & np.isfinite(df).all(1) & np.isfinite(nodf).all(1)
    oo, dd = dot32(p0, p0), dot32(d1, d1)
    return fin & (oo <= T["o2max"]) & (dd >= T["d2min"]) & (dd <= T["d2max"])


def condition2(T, p0, d1, un1):
    """Ray 1 fails the slab test of the box of the class of the smallest value >= un1 (true where there is no such class)."""
    ok = np.ones(len(p0), bool)
    chosen = np.full(len(p0), -1)
    for c in range(int(T["n_classes"]) - 1, -1, -1):
        chosen = np.where(T["class_val"][c] >= un1, c, chosen)
    for c in range(int(T["n_classes"])):
        sel = np.flatnonzero(chosen == c)
        if len(sel):
            box = np.broadcast_to(T["class_box"][c], (len(sel), 6))
            ok[sel] = ~slab_passes(box, p0[sel], d1[sel])
    return ok


def ray2_margin(T, em, nd):
    """(amin, margin) of the emitters' box for the directions +-nd: amin = inf where every emitter rejects by its determinant."""
    amin = np.full(len(nd), np.inf, f32)
    zero = np.zeros_like(nd)
    for v0, v1, v2 in em:
        _, a = mt_accepts(zero, nd, np.broadcast_to(v0, nd.shape), np.broadcast_to(v1, nd.shape), np.broadcast_to(v2, nd.shape))
        amin = np.where(~((a > -EPS) & (a < EPS)), np.minimum(amin, np.abs(a)), amin)
    with np.errstate(all="ignore"):
        m = T["em_rho"] * (float(EPS) / amin.astype(np.float64)) + T["em_add"]
    return amin, m


def condition3(T, em, p0, d1, nd):
    nn = dot32(nd, nd)
    amin, m = ray2_margin(T, em, nd)
    geo = halfplane_misses_box(p0, d1, nd, T["em_lo"], T["em_hi"], np.where(np.isfinite(amin), m, 0.0))
    return (nn >= T["d2min"]) & (nn <= T["d2max"]) & (np.isinf(amin) | (np.isfinite(amin) & geo))


def culled(T, em, p0, d1, un1, nd):
    """The kernel's decision for scattered first-bounce rays (p0, d1) whose generators go on with n1 (as unit_float) and nd =
    randomVector(n1, n2).  em: [(v0, v1, v2)] of the emitters, float32."""
    if not T["on"]:
        return np.zeros(len(p0), bool)
    c1 = np.ones(len(p0), bool)
    for v0, v1, v2 in em:
        acc, _ = mt_accepts(p0, d1, np.broadcast_to(v0, p0.shape), np.broadcast_to(v1, p0.shape), np.broadcast_to(v2, p0.shape))
        c1 &= ~acc
    return ray_in_limits(T, p0, d1) & c1 & condition2(T, p0, d1, un1) & condition3(T, em, p0, d1, nd)


def emitters_of(tris):
    """[(v0, v1, v2)] of the triangles (oracle records) whose emission is not bitwise +0."""
    out = []
    for t in tris:
        e = (f32(t["emissive"]) * t["emit"].astype(f32)).astype(f32)
        if e.view(np.uint32).any():
            out.append((t["a"].astype(f32), t["b"].astype(f32), t["c"].astype(f32)))
    return out


def frame_first_bounces(ob, flat, cam, spp, w, h):
    """Every sample of the w x h frame at spp whose depth-0 bounce scatters off a non-absorbing surface -- what sq_gen_bounce1 would
    queue as ray 1 -- as arrays: y, x, k, p0, d1, n1, n2 (scatterRay as tests/depth_restatement.py walks it)."""
    from depth_restatement import cross, dot, random01, signum
    L = O.lib()
    rows = []
    for y in range(w):
        for x in range(h):
            o, d = O.make_ray(w, h, y, x, cam)
            o, d = np.asarray(o, f32), np.asarray(d, f32)
            hit = ob.intersect(o, d)
            if not hit.hit:
                continue
            t = flat[hit.tri]
            if not t["surf"].any():                                  # absorbs: no ray
                continue
            nrm = cross((t["b"] + -t["a"]).astype(f32), (t["c"] + -t["a"]).astype(f32))
            p0 = np.array([hit.point.x, hit.point.y, hit.point.z], f32)
            for k in range(spp):
                words = O.tfgen_words(spp * (x + y * w) + k)
                if not (t["reflective"] < random01(words[0])):
                    continue
                v = L.sqo_random_vector(words[0], words[1], 0)
                nd = np.array([v.x, v.y, v.z], f32)
                if signum(dot(d, nrm)) == signum(dot(nd, nrm)):
                    nd = -nd
                rows.append((y, x, k, p0, nd, words[1], words[2]))
    cols = list(zip(*rows)) or [()] * 7                                  # no first-bounce ray: empty arrays of the same dtypes and ranks
    return {"y": np.array(cols[0], np.int64), "x": np.array(cols[1], np.int64), "k": np.array(cols[2], np.int64),
            "p0": np.array(cols[3], f32).reshape(-1, 3), "d1": np.array(cols[4], f32).reshape(-1, 3),
            "n1": np.array(cols[5], np.uint32), "n2": np.array(cols[6], np.uint32)}


def frame_prediction(sqt, T, ob, flat, cam, spp, w, h):
    """(first-bounce rays, mask of the culled ones) of a frame."""
    fb = frame_first_bounces(ob, flat, cam, spp, w, h)
    nd = random_vectors(fb["n1"], fb["n2"])
    return fb, culled(T, emitters_of(flat), fb["p0"], fb["d1"], unit_float(fb["n1"]), nd)


def soup(seed, n_emit, n=300, reflective=(0.0, 0.1, 0.3, 0.5, 0.8, 1.0), emit=(1.0, 0.8, 0.6), spread=0.35, emitter_size=None, cluster=None, zoned=None):
    """A random triangle soup: materials 0 .. len(reflective)-1 diffuse / partly / always mirroring, the last material the lamp's
    (absorbing, emissive), on n_emit triangles -- random ones, or (cluster = a point) the ones nearest to that point, so that the
    emitters' box is a corner of the scene.  zoned = a point: only the sixth of the triangles nearest to it get a non-zero `reflective`
    (mirrors everywhere would put every ray 1 inside the box of its mirror class).  Returns (tris, mats, oracle triangle records)."""
    N = importlib.import_module("squigly-trace_amd._native")
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1.5, 1.5, (n, 1, 3))
    v = (c + rng.normal(0, spread, (n, 3, 3))).astype(f32)
    nm = len(reflective)
    mats = np.zeros(nm + 1, N.MAT_DTYPE)
    mats["reflective"][:nm] = reflective
    mats["surf"][:nm] = rng.uniform(0.2, 0.9, (nm, 3))
    mats["emissive"][nm] = 25
    mats["emit"][nm] = emit
    mat = rng.integers(0, nm, n)
    if zoned is not None:
        mat[np.argsort(np.linalg.norm(c[:, 0] - np.asarray(zoned), axis=1))[n // 6:]] = 0
    em = rng.choice(n, n_emit, replace=False)
    if cluster is not None:
        em = np.argsort(np.linalg.norm(c[:, 0] - np.asarray(cluster), axis=1))[:n_emit]
    mat[em] = nm
    if emitter_size is not None:
        v[em] = (c[em] + rng.normal(0, emitter_size, (n_emit, 3, 3))).astype(f32)
    if n_emit:                                                           # an emitter that shares an edge with a diffuse triangle, and one grazing it
        a, b = em[0], np.flatnonzero(mat != nm)[0]
        v[b, 0], v[b, 1] = v[a, 1], v[a, 0]
        v[b, 2] = v[a, 2] + f32(1e-4) * rng.normal(0, 1, 3).astype(f32)
    tris = np.zeros(n, N.TRI_DTYPE)
    tris["v0"], tris["v1"], tris["v2"], tris["mat"] = v[:, 0], v[:, 1], v[:, 2], mat
    ot = np.zeros(n, O.TRI_DTYPE)
    ot["a"], ot["b"], ot["c"] = v[:, 0], v[:, 1], v[:, 2]
    for f in ("reflective", "surf", "emissive", "emit"):
        ot[f] = mats[f][mat]
    return tris, mats, ot


# The soups more than one file names: the counter-example searches of tests/test_level1_cull.py ("soup", "soup_big_emitters": few
# emitters, so that their box is not the whole soup and rays aimed beside them can be culled at all) and tests/test_level1_stretch.py
# (the other three), and the recorded level-1 records of tests/test_pack.py.
NAMED_SOUPS = {"soup": lambda: soup(12, 1),
               "soup_big_emitters": lambda: soup(11, 2, emitter_size=0.9, cluster=(1.2, 1.2, -1.2)),
               "one": lambda: soup(41, 1, zoned=(1.2, -1.2, -1.2), emitter_size=0.8),
               "two_clustered": lambda: soup(42, 2, zoned=(-1.2, -1.2, -1.2), cluster=(1.2, 1.2, -1.2), emitter_size=0.6),
               "many_clustered": lambda: soup(43, 12, zoned=(1.2, -1.2, -1.2), cluster=(-1.0, 1.0, 1.0))}
