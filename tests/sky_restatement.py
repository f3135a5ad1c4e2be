"""Lib.raytrace under a path depth D and a caller-given sky (sq_scene_set_sky), restated in numpy float32 from the oracle's primitives.

include/squigly_hip.h's chain with one line changed: a ray that intersects nothing returns sky(d) of its direction as traced, where
depth_restatement (and the reference) say black.  The walk is depth_restatement.path itself, told to keep the direction of the ray
that missed (`Miss`) where it would end a path on None.  tests/test_sky.py pins this module to depth_restatement
-- and through it to the oracle -- with no sky, and judges what the shared inputs cover; tests/test_gpu_sky.py holds the kernels to it.

A sky is None or (up, down), three float32 each."""
import functools
import os

import numpy as np
import pyoracle as O

import depth_restatement as DR
from scenes import ROTATED

f32 = np.float32
MAX_DEPTH = DR.MAX_DEPTH
GRADIENT = ((0.25, 0.5, 1.0), (0.75, 0.625, 0.5))       # up, down: every channel differs, and up differs from down in every channel
CONSTANT = (GRADIENT[0], GRADIENT[0])


class Miss:
    """The end of a path on a ray that hits nothing: d = that ray's direction, exactly as it was traced."""

    def __init__(self, d):
        self.d = np.asarray(d, f32).copy()


def sky_t(d):
    """n = sqrt((d.x*d.x + d.y*d.y) + d.z*d.z);  u = d.z / n;  t = 0.5 * u + 0.5 -- every operation a single float32 operation."""
    d = np.asarray(d, f32)
    with np.errstate(all="ignore"):
        n = f32(np.sqrt(f32(f32(f32(d[0] * d[0]) + f32(d[1] * d[1])) + f32(d[2] * d[2]))))
        u = f32(d[2] / n)
        return f32(f32(f32(0.5) * u) + f32(0.5))


def sky_of(sky, d):
    """sky_c = down_c + t * (up_c - down_c)."""
    up, down = np.asarray(sky[0], f32), np.asarray(sky[1], f32)
    t = sky_t(d)
    with np.errstate(all="ignore"):
        return (down + (t * (up - down).astype(f32)).astype(f32)).astype(f32)


def path(ob, flat, words, o, d, depth=MAX_DEPTH):
    """depth_restatement.path with the miss kept: the triangles the rays 0 .. depth-1 hit, a Miss where the path ends on one."""
    return DR.path(ob, flat, words, o, d, depth, miss=Miss)


def radiance(trail, depth, sky):
    """L(0) of the path cut at `depth` under `sky`: the fold from the innermost level outwards, starting from black where the depth
    ends the path and from sky(d) where a ray misses; the product with either is formed at the innermost hit."""
    rad = np.zeros(3, f32)
    with np.errstate(all="ignore"):
        for t in reversed(trail[:depth]):
            if isinstance(t, Miss):
                rad = np.zeros(3, f32) if sky is None else sky_of(sky, t.d)
            else:
                rad = ((t["surf"] * rad).astype(f32) + (t["emissive"] * t["emit"]).astype(f32)).astype(f32)
    return rad


def paths(ob, flat, o, d, seeds, k=0, depth=MAX_DEPTH):
    return DR.paths(ob, flat, o, d, seeds, k, depth, miss=Miss)


def radiances(trails, depth, sky):
    return np.array([radiance(t, depth, sky) for t in trails], f32).reshape(len(trails), 3)


def miss_level(trail, depth=MAX_DEPTH):
    """The level at which the path, cut at `depth`, ends on a miss; None when it does not."""
    cut = trail[:depth]
    return len(cut) - 1 if cut and isinstance(cut[-1], Miss) else None


def absorbing_above_miss(trail, depth):
    """Does the path, cut at `depth`, end on a miss with a surfColor == 0 hit above it (where 0 * sky is formed)?"""
    m = miss_level(trail, depth)
    return m is not None and any((t["surf"] == 0).all() for t in trail[:m])


def frame_paths(ob, flat, cam, spp, w, h, rows=None):
    """depth_restatement.frame_paths with the misses kept."""
    return DR.frame_paths(ob, flat, cam, spp, w, h, rows, miss=Miss)


def fold_frame(trails_by_sample, depth, sky, n=None, start=None, start2=None):
    """(sum, sum2, avg) over the samples, in order, as depth_restatement.fold_frame; start / start2: where the folds begin."""
    s = np.zeros((len(trails_by_sample[0]), 3), f32) if start is None else np.array(start, f32).reshape(-1, 3)
    q = np.zeros_like(s) if start2 is None else np.array(start2, f32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        for trails in trails_by_sample:
            r = radiances(trails, depth, sky)
            s = (s + r).astype(f32)
            q = (q + (r * r).astype(f32)).astype(f32)
        avg = ((f32(1) / f32(n if n is not None else len(trails_by_sample))) * s).astype(f32)
    return s, q, avg


# ---- the inputs the sky tests share: depth_restatement's cases and fuzz_features'.  Their one walk is made here, with the misses
# ---- kept; the depth view of it reads each Miss as None (depth_restatement.plain) -----------------------------------------------
def case_paths(c, k=0):
    """The paths of a depth_restatement.case's rays under the generators mkTFGen (seed + k), walked once."""
    if not hasattr(c, "sky_paths"):
        c.sky_paths = {}
    if k not in c.sky_paths:
        c.sky_paths[k] = paths(c.ob, c.flat, c.o, c.d, c.s, k=k)
    return c.sky_paths[k]


@functools.lru_cache(maxsize=None)
def frame_case(which, camera, w, h, spp):
    c = DR.case(which)
    text = open(os.path.join(DR.DATA, "camera"), "rb").read() if camera == "camera" else ROTATED
    return frame_paths(c.ob, c.flat, O.camera_from_text(text), spp, w, h)


# ---- random scenes: fuzz_features.case(seed) and a sky of its own ----------------------------------------------------------------
def fuzz_sky(seed):
    """The sky of seed N, from a generator of its own, default_rng([N, 2]) (fuzz_features.case draws from [N, 1]): up and down in
    [0, 2), one seed in eight a constant sky, one in eight with a component that is inf, negative, NaN or zero."""
    rng = np.random.default_rng([seed, 2])
    up, down = rng.uniform(0, 2, 3).astype(f32), rng.uniform(0, 2, 3).astype(f32)
    kind = rng.random()
    if kind < 0.125:
        down = up.copy()
    elif kind < 0.25:
        (up if rng.random() < 0.5 else down)[int(rng.integers(0, 3))] = rng.choice([np.inf, -1.5, np.nan, 0.0])
    return tuple(float(v) for v in up), tuple(float(v) for v in down)


def fuzz_frame_paths(c, second=False):
    """frame_paths of a fuzz_features case's shard under its first or second camera, walked once."""
    key = "_sky_paths2" if second else "_sky_paths"
    if not hasattr(c, key):
        setattr(c, key, frame_paths(c.ob, c.flat, c.ocam2 if second else c.ocam, c.spp, c.w, c.h, rows=c.rows))
    return getattr(c, key)


def fuzz_ray_paths(c):
    import fuzz_features as FF
    if not hasattr(c, "_sky_ray_paths"):
        o, d, s = FF.radiance_rays(c)
        c._sky_ray_paths = paths(c.ob, c.flat, o, d, s)
    return c._sky_ray_paths
