"""Arithmetic of the kernels restated in numpy, shared by the culling lemmas (tests/test_cull.py, tests/test_level1_cull.py), the
padding and level-1 restatements built on them and the planner's tests.

Belongs here: a test or an enumeration the device code performs, written as the kernels compute it (operation order, one rounding
per operation), and the rays made to probe it.  Needs no GPU and no native library."""
import numpy as np

f32 = np.float32


def mt_accepts(o, d, v0, v1, v2):
    """mollerTrumbore in float32, vectorised over rows; the reference's operation order (src/V3.hs dot/cross)."""
    def dot(a, b): return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]
    def cross(a, b): return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
    eps = f32(0.0001)
    e1, e2 = v1 - v0, v2 - v0
    h = cross(d, e2)
    a = dot(e1, h)
    with np.errstate(all="ignore"):
        f = f32(1) / a
        s = o - v0
        u = f * dot(s, h)
        q = cross(s, e1)
        v = f * dot(d, q)
        t = f * dot(e2, q)
        return ~((a > -eps) & (a < eps)) & ~((u < 0) | (u > 1)) & ~((v < 0) | (u + v > 1)) & (t > eps), a


def fma32(a, b, c):
    """fl32(a * b + c) with ONE rounding, for float32 arrays -- exactly what v_fma_f32 / v_fma_mix_f32 return.
    a * b is exact in binary64 (24 + 24 bits); the sum is taken with TwoSum, and the binary64 sum is turned into the
    round-to-odd value of the exact result (if inexact, whichever neighbour has an odd last bit), which then rounds to
    binary32 as the exact value would (53 >= 24 + 2: no double rounding).  x86 long double (64-bit significand, the first
    version of this test) is NOT enough: its own rounding can land on a binary32 midpoint."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = np.broadcast_to(c.astype(np.float64), p.shape)
    with np.errstate(all="ignore"):
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)                      # exact: s + err == p + c
    fin = np.isfinite(s) & np.isfinite(err) & (err != 0)
    bits = s.view(np.int64).copy() if s.flags.writeable else s.copy().view(np.int64)
    even = (bits & 1) == 0
    toward_larger_magnitude = (err > 0) == (s > 0)           # exact value lies on this side of s
    adj = fin & even
    # for s == 0 (cannot happen with err != 0: the sum of two finite doubles that rounds to 0 is exact) nothing to do
    step = np.where(toward_larger_magnitude, 1, -1)
    bits = np.where(adj, bits + step, bits)
    return bits.view(np.float64).astype(np.float32)


def slab_passes(box, o, d):
    """The kernels' culling slab test: plane value = fma(l, 1/d, -o * (1/d)) with one rounding, v_min/v_max, tmax > 0 && tmin < tmax."""
    with np.errstate(all="ignore"):
        df = f32(1) / d
        nodf = -o * df
        tl = fma32(box[:, 0:3], df, nodf)
        th = fma32(box[:, 3:6], df, nodf)
    tmin = np.minimum(tl, th).max(1)
    tmax = np.maximum(tl, th).min(1)
    return (tmax > 0) & (tmin < tmax)


def grazing_rays(rng, tris, n, omax, eps_scale):
    """Rays nearly parallel to a triangle's plane, aimed at a point just outside (or inside) one of its edges or corners."""
    k = rng.integers(0, len(tris), n)
    v0, v1, v2 = (tris[f][k].astype(np.float64) for f in ("v0", "v1", "v2"))
    e1, e2 = v1 - v0, v2 - v0
    nrm = np.cross(e1, e2)
    area2 = np.linalg.norm(nrm, axis=1)
    good = area2 > 1e-12
    nrm = nrm / np.maximum(area2, 1e-300)[:, None]
    # target point: barycentric (u, v) on an edge or a corner, pushed outwards by a log-uniform amount
    kind = rng.integers(0, 6, n)
    lam = rng.random(n)
    bu = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4, kind == 5], [lam, 0 * lam, lam, 0 * lam, 1 + 0 * lam, 0 * lam])
    bv = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4, kind == 5], [0 * lam, lam, 1 - lam, 0 * lam, 0 * lam, 1 + 0 * lam])
    push = 10.0 ** rng.uniform(-9, -1.5, n) * rng.choice([-1.0, 1.0], n)
    cen = (v0 + v1 + v2) / 3
    tgt = v0 + bu[:, None] * e1 + bv[:, None] * e2
    out = tgt - cen
    out /= np.maximum(np.linalg.norm(out, axis=1), 1e-300)[:, None]
    tgt = tgt + push[:, None] * out
    # direction: in-plane unit vector tilted so that |a| = |d . (e1 x e2)| is a small multiple of the test's epsilon
    ang = rng.uniform(0, 2 * np.pi, n)
    t1 = e1 / np.maximum(np.linalg.norm(e1, axis=1), 1e-300)[:, None]
    t2 = np.cross(nrm, t1)
    inpl = np.cos(ang)[:, None] * t1 + np.sin(ang)[:, None] * t2
    want_a = 1e-4 * 10.0 ** rng.uniform(0, eps_scale, n) * rng.choice([-1.0, 1.0], n)
    tilt = np.clip(want_a / np.maximum(area2, 1e-300), -0.9, 0.9)
    d = inpl * np.sqrt(1 - tilt ** 2)[:, None] + tilt[:, None] * nrm
    d *= rng.uniform(0.8, 1.2, n)[:, None]                      # |d| in [0.8, 1.2]: inside the limits
    dist = rng.uniform(0.01, 1.0, n) * omax
    o = tgt - dist[:, None] * d / np.linalg.norm(d, axis=1)[:, None]
    return k[good], o[good].astype(f32), d[good].astype(f32)


def tile_rows_for(n_shards, row_block):
    """Rows of a primary tile (primary_tile in the device code): 8 for a whole frame, else the largest of 8, 4, 2, 1 dividing row_block."""
    rb = 8 if n_shards <= 1 else row_block
    return 8 if rb >= 8 and rb % 8 == 0 else 4 if rb >= 4 and rb % 4 == 0 else 2 if rb >= 2 and rb % 2 == 0 else 1


def enumerate_pixels(local_rows, h, tile_rows):
    """(pixel of every padded position q, or -1 for padding; the padded count) of the tiled enumeration of the primary rays."""
    tw = 64 // tile_rows
    tiles_x = (h + tw - 1) // tw
    padded = ((local_rows + tile_rows - 1) // tile_rows) * tiles_x * 64
    q = np.arange(padded, dtype=np.int64)
    lane, tile = q & 63, q >> 6
    ty, tx = tile // tiles_x, tile % tiles_x
    jj, xx = lane // tw, lane % tw
    j, x = ty * tile_rows + jj, tx * tw + xx
    ok = (j < local_rows) & (x < h)
    return np.where(ok, j * h + x, -1), padded
