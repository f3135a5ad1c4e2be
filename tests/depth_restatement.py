"""Lib.raytrace (src/Lib.hs:127-137) under a path depth D, restated in numpy float32 from the oracle's primitives.

The oracle is fixed at depth 3 (`bounces > 2 = black`, src/Lib.hs:129), so the depth tests cannot ask it for another depth.  What they
hold the kernels to is this restatement of include/squigly_hip.h's formula -- intersectBIH, the generator words and randomVector come
from the oracle, every other operation is a single float32 operation written out here -- and tests/test_depth.py pins it to the oracle
itself at D = 3: sqo_sample_radiance bit for bit on the rays the GPU tests use, sqo_render on a frame.

A path does not depend on the depth it is cut at: `path` walks it once to the largest depth and `radiance` folds any prefix of it.
Nor does it depend on what a miss is worth: `path` is also sky_restatement's walk, which keeps the direction of the ray that missed
(`miss`), and the shared inputs below are walked once, for both modules."""
import functools
import importlib
import os

import numpy as np
import pyoracle as O

from ray_oracle import make_radiance_families
from scenes import BRIGHT_SQ

f32 = np.float32
MAX_DEPTH = 8


def dot(p, q):
    return f32(f32(f32(p[0] * q[0]) + f32(p[1] * q[1])) + f32(p[2] * q[2]))


def cross(p, q):
    a, b, c = p
    d, e, f = q
    return np.array([f32(f32(b * f) - f32(c * e)), f32(f32(c * d) - f32(a * f)), f32(f32(a * e) - f32(b * d))], f32)


def signum(x):
    return f32(1) if x > 0 else (f32(-1) if x < 0 else x)


def random01(n):
    return f32(f32(0) + f32(f32(1) * f32(f32(n) / f32(4294967296.0))))


def path(ob, flat, words, o, d, depth=MAX_DEPTH, miss=None):
    """The triangles (records of flat = ob.flatten()) the rays 0 .. depth-1 of a path hit; where the path ends on a miss, None, or
    miss(d) of the direction of the ray that missed, exactly as it was traced.
    ob: pyoracle.BIH; words = pyoracle.tfgen_words(seed); o, d: ray 0."""
    L = O.lib()
    trail = []
    o, d = np.asarray(o, f32), np.asarray(d, f32)
    with np.errstate(all="ignore"):
        for b in range(depth):
            h = ob.intersect(o, d)
            if not h.hit:
                trail.append(None if miss is None else miss(d))
                break
            t = flat[h.tri]
            trail.append(t)
            if b + 1 >= depth:
                break
            nrm = cross((t["b"] + -t["a"]).astype(f32), (t["c"] + -t["a"]).astype(f32))
            if t["reflective"] < random01(words[b]):
                v = L.sqo_random_vector(words[b], words[b + 1], 0)
                nd = np.array([v.x, v.y, v.z], f32)
                if signum(dot(d, nrm)) == signum(dot(nd, nrm)):
                    nd = -nd
            else:
                dn = (nrm / f32(np.sqrt(dot(nrm, nrm)))).astype(f32)
                nd = (d + -(f32(f32(2) * dot(dn, d)) * dn).astype(f32)).astype(f32)
            o, d = np.array([h.point.x, h.point.y, h.point.z], f32), nd
    return trail


def radiance(trail, depth):
    """L(0) of the path cut at `depth`: the fold from the innermost level outwards, the product with black formed there."""
    rad = np.zeros(3, f32)
    with np.errstate(all="ignore"):
        for t in reversed(trail[:depth]):
            rad = np.zeros(3, f32) if t is None else ((t["surf"] * rad).astype(f32) + (t["emissive"] * t["emit"]).astype(f32)).astype(f32)
    return rad


def raytrace(ob, flat, words, o, d, depth):
    return radiance(path(ob, flat, words, o, d, depth), depth)


def paths(ob, flat, o, d, seeds, k=0, depth=MAX_DEPTH, miss=None):
    """The path of every ray i with the generator mkTFGen (seeds[i] + k)."""
    return [path(ob, flat, O.tfgen_words(int(seeds[i]) + k), o[i], d[i], depth, miss) for i in range(len(o))]


def plain(trails):
    """Paths walked with their misses kept (`miss`), read as paths walked without: None wherever one holds no triangle record."""
    return [[t if isinstance(t, np.void) else None for t in trail] for trail in trails]


def radiances(trails, depth):
    return np.array([radiance(t, depth) for t in trails], f32).reshape(len(trails), 3)


def frame_paths(ob, flat, cam, spp, w, h, rows=None, miss=None):
    """paths[k][j * h + x] of sample k of pixel (y, x) of the spp-sample frame, y over `rows` (default: all w rows); the seed is
    spp * (x + y * w) + k (src/Lib.hs:85)."""
    rows = range(w) if rows is None else rows
    rays = [(y, x) + O.make_ray(w, h, y, x, cam) for y in rows for x in range(h)]
    return [[path(ob, flat, O.tfgen_words(spp * (x + y * w) + k), o, d, miss=miss) for (y, x, o, d) in rays] for k in range(spp)]


def fold_frame(trails_by_sample, depth, n=None):
    """(sum, sum2, avg) over the samples, in order: sum = sum + r, sum2 = sum2 + r * r, avg = (1 / n) *^ sum (n: the frame's k_end)."""
    s = np.zeros((len(trails_by_sample[0]), 3), f32)
    q = np.zeros_like(s)
    with np.errstate(all="ignore"):
        for trails in trails_by_sample:
            r = radiances(trails, depth)
            s = (s + r).astype(f32)
            q = (q + (r * r).astype(f32)).astype(f32)
        avg = ((f32(1) / f32(n if n is not None else len(trails_by_sample))) * s).astype(f32)
    return s, q, avg


# ---- the inputs the depth tests share (tests/test_depth.py judges them, tests/test_gpu_depth.py runs them) -----------------------
DATA = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data")
N_RAYS = 1000                      # per family
FAMILIES = ("free", "surface", "to_light", "degenerate")
BIG = b"1" + b"0" * 40             # reads as +inf in float32


def odd_sq():
    """The bright materials with an infinite `emissive`, a negative surfColor component and a zero surfColor (the lamp's): not every
    component is >= +0, so the exact shortcuts for absorbing surfaces are off, and inf * 0 = NaN reaches the folds."""
    sq = BRIGHT_SQ.replace(b"emissive 0.5 0.3 0.6 0.9", b"emissive " + BIG + b" 0.3 0.6 0.9")
    sq = sq.replace(b"reflective 0.2 0.608420 0.508420 0.408420", b"reflective 0.2 0.608420 -0.508420 0.408420")
    assert sq.count(BIG) == 1 and b"-0.508420" in sq and b"reflective 0 0 0 0" in sq
    return sq


class Case:
    """One material set on data/scene.obj: product BIH, oracle BIH and its flattened triangles, and N_RAYS rays per family with seeds
    that are small, huge and negative (ray_oracle.make_radiance_families), each with its path to MAX_DEPTH.
    The "free" family here is the first N_RAYS free rays of the generator whose ray 0 hits the scene: 38 % of the generator's free rays
    start outside the open room and hit nothing, which is black at every depth -- the other three families keep their misses."""


def first_hitting(ob, o, d, n):
    """Indices of the first n rays that intersectBIH hits."""
    idx = []
    for i in range(len(o)):
        if ob.intersect(o[i], d[i]).hit:
            idx.append(i)
            if len(idx) == n:
                break
    assert len(idx) == n, (len(idx), n)
    return np.array(idx)


@functools.lru_cache(maxsize=None)
def case(which):
    sqt = importlib.import_module("squigly-trace_amd")
    obj = open(os.path.join(DATA, "scene.obj"), "rb").read()
    sq = {"bright": lambda: BRIGHT_SQ, "shipped": lambda: open(os.path.join(DATA, "scene.sq"), "rb").read(), "odd": odd_sq}[which]()
    c = Case()
    c.which = which
    c.bih = sqt.BIH(sqt.Mesh.from_text(obj, sq))
    c.otris = O.tris_from_text(obj, sq)
    c.ob = O.BIH(c.otris)
    c.flat = c.ob.flatten()
    fam, seeds = make_radiance_families(c.bih, c.flat, {"bright": 12, "shipped": 11, "odd": 13}[which])
    keep = FAMILIES if which != "odd" else ("free",)
    n = N_RAYS if which != "odd" else 500
    c.families = keep
    c.n = n
    pick = {k: first_hitting(c.ob, *fam[k], n) if k == "free" else np.arange(n) for k in keep}
    c.o = np.ascontiguousarray(np.concatenate([fam[k][0][pick[k]] for k in keep]), f32)
    c.d = np.ascontiguousarray(np.concatenate([fam[k][1][pick[k]] for k in keep]), f32)
    c.s = np.ascontiguousarray(np.concatenate([seeds[k][pick[k]] for k in keep]), np.int64)
    c.paths = {}
    return c


def case_paths(c, k=0):
    """The paths of the case's rays under the generators mkTFGen (seed + k), walked once: sky_restatement.case_paths' walk, which
    keeps the misses, with each Miss read as None."""
    import sky_restatement as SR                                        # (it imports this module)
    if k not in c.paths:
        c.paths[k] = plain(SR.case_paths(c, k))
    return c.paths[k]


@functools.lru_cache(maxsize=None)
def frame_case(which, camera, w, h, spp):
    """frame_paths of the whole w x h frame at spp samples under data/camera ("camera") or the rotated camera: sky_restatement.frame_case's
    walk with each Miss read as None."""
    import sky_restatement as SR
    return [plain(trails) for trails in SR.frame_case(which, camera, w, h, spp)]


def shard_rows(w, shard):
    """The global rows of a shard (row_block, index, n_shards), in local order; (None, 0, 1) is every row."""
    rb, si, ns = shard
    if rb is None:
        return list(range(w))
    return [y for y in range(w) if (y // rb) % ns == si]
