"""Condition (4) of level-1 culling (squigly-trace_amd/csrc/sq_pack_level1.h, build_level1 and level1_cover; sq_kernels_wave.h,
stretch_misses_cover) restated in numpy, on top of tests/level1_restatement.py.

A sample that conditions (1) and (2) pass and (3) keeps is still culled when the stretch [ta, tb] of ray 1 -- the t >= 0 from whose
points p0 + t d1 the line along nd reaches the emitters' grown box -- is empty, or misses, for every box of the cover (packed array
"level1_cover"), ray 1's slab interval widened by the box's r |t| + c.  The stretch is evaluated in binary64 with the kernel's
operation order, the slab intervals in float32 with single-rounding FMAs (tests/kernel_restatements.py)."""
import ctypes as C

import numpy as np

import level1_restatement as R
from kernel_restatements import fma32, mt_accepts

f32 = np.float32
COVER = np.dtype({"names": ["n", "r", "c", "box"], "formats": ["<i4", ("<f4", 8), ("<f4", 8), ("<f4", (8, 6))], "offsets": [0, 16, 48, 80], "itemsize": 272})


def cover(sqt, holder):
    """The Level1Cover record of holder.scene through sq_scene_pack, or None where the packer wrote none (level1_on = 0)."""
    L, h = sqt.lib(), C.c_void_p()
    sqt._native.check(L.sq_scene_pack(C.byref(holder.scene), C.byref(h)))
    try:
        data, n = C.c_void_p(), C.c_size_t()
        assert L.sq_packed_array(h, b"level1_cover", C.byref(data), C.byref(n)) == 0
        if n.value == 0:
            return None
        assert n.value == COVER.itemsize, n.value
        return np.frombuffer(C.string_at(data, n.value), COVER)[0]
    finally:
        L.sq_packed_free(h)


def stretch(p0, d1, nd, lo, hi, m):
    """(ta, tb) as the kernel computes them: the intersection of [0, inf) with the three slabs |t N_k - G_k| <= r_k + tol."""
    p, d, n = p0.astype(np.float64), d1.astype(np.float64), nd.astype(np.float64)
    g = 0.5 * (lo + hi)[None, :] - p
    h = 0.5 * (hi - lo)[None, :] + m[:, None]
    scale = np.zeros(len(p))
    for k in range(3):
        scale = scale + (np.abs(g[:, k]) + h[:, k])
    tol = 1e-9 * scale
    N = [d[:, 1] * n[:, 2] - d[:, 2] * n[:, 1], d[:, 2] * n[:, 0] - d[:, 0] * n[:, 2], d[:, 0] * n[:, 1] - d[:, 1] * n[:, 0]]
    G = [g[:, 1] * n[:, 2] - g[:, 2] * n[:, 1], g[:, 2] * n[:, 0] - g[:, 0] * n[:, 2], g[:, 0] * n[:, 1] - g[:, 1] * n[:, 0]]
    a = np.abs(n)
    r = [a[:, 2] * h[:, 1] + a[:, 1] * h[:, 2], a[:, 2] * h[:, 0] + a[:, 0] * h[:, 2], a[:, 1] * h[:, 0] + a[:, 0] * h[:, 1]]
    ta, tb = np.zeros(len(p)), np.full(len(p), np.inf)
    with np.errstate(all="ignore"):
        use = [np.abs(N[k]) >= 1e-6 for k in range(3)]
        Nu = [np.where(use[k], N[k], 1.0) for k in range(3)]
        inv = 1.0 / ((Nu[0] * Nu[1]) * Nu[2])                            # one division: 1 / N_k = (the other two) / (all three)
        rc = [inv * (Nu[1] * Nu[2]), inv * (Nu[0] * Nu[2]), inv * (Nu[0] * Nu[1])]
        for k in range(3):
            w = r[k] + tol
            q1, q2 = (G[k] - w) * rc[k], (G[k] + w) * rc[k]
            ql, qh = np.minimum(q1, q2), np.maximum(q1, q2)
            ta = np.where(use[k], np.maximum(ta, ql - 1e-9 * np.abs(ql)), ta)
            tb = np.where(use[k], np.minimum(tb, qh + 1e-9 * np.abs(qh)), tb)
    return ta, tb


def slab_interval(box, o, d):
    """(tmin, tmax) of the kernels' float32 slab test of one box (lo.xyz, hi.xyz) for the rays (o, d)."""
    box = np.broadcast_to(box, (len(o), 6))
    with np.errstate(all="ignore"):
        df = f32(1) / d
        nodf = -o * df
        tl = fma32(box[:, 0:3], df, nodf)
        th = fma32(box[:, 3:6], df, nodf)
    return np.minimum(tl, th).max(1), np.maximum(tl, th).min(1)


def stretch_misses_cover(V, p0, d1, nd, lo, hi, m, use_cover=True, why=None):
    """The kernel's condition (4).  V: the cover record or None; use_cover = False: the stretch alone (part (a) of the condition).
    why = a dict: it receives the two alternatives per row, "empty" (no stretch) and "may_end" (ray 1 may end in a box of the cover, at
    a point of the stretch)."""
    ta, tb = stretch(p0, d1, nd, lo, hi, m)
    empty = ta > tb
    if why is not None:
        why.update(empty=empty, may_end=np.ones(len(p0), bool))
    if V is None or not use_cover or int(V["n"]) == 0:
        return empty
    with np.errstate(all="ignore"):
        ta32 = np.where(ta > 1e-30, (ta * (1.0 - 2.0 ** -20)).astype(f32), f32(0))
        tb32 = (tb * (1.0 + 2.0 ** -20)).astype(f32)
    may_end = np.zeros(len(p0), bool)
    for j in range(8):                                                   # the kernel reads every entry; those beyond n repeat the first
        tmin, tmax = slab_interval(V["box"][j], p0, d1)
        with np.errstate(all="ignore"):                                  # t^ lies within r |t| + c of a t in [tmin, tmax]: float32, one rounding each
            tlo = (tmin - V["r"][j] * np.abs(tmin)) - V["c"][j]
            thi = (tmax + V["r"][j] * np.abs(tmax)) + V["c"][j]
            may_end |= np.fmax(tlo, ta32) <= np.fmin(thi, tb32)          # v_max_f32 / v_min_f32 return the other operand for a NaN
    if why is not None:
        why.update(may_end=may_end)
    return empty | ~may_end


def culled(T, V, em, p0, d1, un1, nd, use_cover=True, why=None):
    """(culled by conditions (1)-(3), culled by (1), (2) and (4) alone) for scattered first-bounce rays, as level1_restatement.culled
    takes them.  The two masks are disjoint: the kernel evaluates (4) only where (3) keeps the sample.  why = a dict: it receives "rows"
    (the rows (4) judged) and stretch_misses_cover's report for them."""
    old = R.culled(T, em, p0, d1, un1, nd)
    if not T["on"]:
        return old, np.zeros(len(p0), bool)
    c1 = np.ones(len(p0), bool)
    for v0, v1, v2 in em:
        acc, _ = mt_accepts(p0, d1, np.broadcast_to(v0, p0.shape), np.broadcast_to(v1, p0.shape), np.broadcast_to(v2, p0.shape))
        c1 &= ~acc
    nn = R.dot32(nd, nd)
    amin, m = R.ray2_margin(T, em, nd)
    reach4 = R.ray_in_limits(T, p0, d1) & c1 & R.condition2(T, p0, d1, un1) & (nn >= T["d2min"]) & (nn <= T["d2max"]) & np.isfinite(amin) & ~old
    new = np.zeros(len(p0), bool)
    sel = np.flatnonzero(reach4)
    if len(sel):
        new[sel] = stretch_misses_cover(V, p0[sel], d1[sel], nd[sel], T["em_lo"], T["em_hi"], m[sel], use_cover, why=why)
        if why is not None:
            why["rows"] = sel
    return old, new


def frame_prediction(sqt, T, V, ob, flat, cam, spp, w, h, use_cover=True):
    """(first-bounce rays, mask culled by (1)-(3), mask culled by (4) alone) of a frame."""
    fb = R.frame_first_bounces(ob, flat, cam, spp, w, h)
    nd = R.random_vectors(fb["n1"], fb["n2"])
    old, new = culled(T, V, R.emitters_of(flat), fb["p0"], fb["d1"], R.unit_float(fb["n1"]), nd, use_cover)
    return fb, old, new
