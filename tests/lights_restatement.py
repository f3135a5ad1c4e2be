"""Caller-given point lights, restated: the formula of include/squigly_hip.h for a cast computation under any lights, in numpy
float32 with the header's parenthesisation, over the oracle's intersectBIH.

Belongs here: what a cast frame or a raycast query is under lights the oracle has no entry point for, and the fold and average of
such a frame.  For the reference's light the restatement is bit-equal to O.BIH.render(..., cast=True) (tests/test_gpu_lights.py,
test_the_reference_light_in_every_spelling; tests/test_fuzz_features.py on every seed of its slice).  Needs no GPU."""
import numpy as np

f32 = np.float32


def norm(v):
    return np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2], dtype=f32)


def as_light(light):
    pos, power = light
    return np.asarray(pos, f32), np.asarray(power, f32)


class Restatement:
    """The header's formula over the oracle's intersectBIH.  Primary hits are computed once per ray set and kept."""

    def __init__(self, O, ob):
        self.O, self.ob, self.flat = O, ob, ob.flatten()
        self._primary = {}

    def primary(self, key, rays):
        """[(hit, point, surf)] of the rays; key names the ray set."""
        if key not in self._primary:
            out = []
            for o, d in rays:
                h = self.ob.intersect(o, d)
                if h.hit:
                    out.append((True, np.array([h.point.x, h.point.y, h.point.z], f32), np.asarray(self.flat[h.tri]["surf"], f32)))
                else:
                    out.append((False, None, None))
            self._primary[key] = out
        return self._primary[key]

    def radiance(self, key, rays, lights):
        """T per ray [n, 3] (zeros for a miss), and lit [n, m]: 1 lit, 0 shadowed, -1 the ray misses."""
        prim = self.primary(key, rays)
        lights = [as_light(li) for li in lights]
        T = np.zeros((len(prim), 3), f32)
        lit = np.full((len(prim), len(lights)), -1, np.int8)
        with np.errstate(all="ignore"):
            for i, (hit, p, surf) in enumerate(prim):
                if not hit:
                    continue
                tot = None
                for j, (pos, power) in enumerate(lights):
                    dl = norm((p - pos).astype(f32))
                    sh = self.ob.intersect(p, (pos - p).astype(f32))
                    is_lit = not (sh.hit and not (f32(sh.dist) > dl))
                    c = ((power / dl).astype(f32) * surf).astype(f32) if is_lit else np.zeros(3, f32)
                    lit[i, j] = int(is_lit)
                    tot = c if tot is None else (tot + c).astype(f32)
                T[i] = tot
        return T, lit


def fold_cast(T, k_begin, k_end, start=None):
    """sum = sum + T per sample of [k_begin, k_end), from +0 or `start`."""
    s = np.zeros_like(T) if start is None else start.copy()
    with np.errstate(all="ignore"):
        for _ in range(k_begin, k_end):
            s = (s + T).astype(f32)
    return s


def avg_of(s, k_end):
    with np.errstate(all="ignore"):
        return ((f32(1) / f32(k_end)) * s).astype(f32)
