"""Condition (5) of level-1 culling (squigly-trace_amd/csrc/sq_pack_level1.h, build_level1 and level1_mirror; sq_kernels_wave.h,
mirror_cannot_reach) restated in numpy, on top of tests/level1_restatement.py and tests/level1_stretch_restatement.py.

A sample whose ray 1 PASSES the box of its mirror class -- condition (2) fails -- is still culled when no triangle that mirrors under n1
can send ray 2 to an emitter (ray 1 misses the rest boxes, keeps every mirrored determinant above the floor, and behind no panel
reaches the image of the emitters' box) and conditions (3) / (4) answer for the triangles that scatter under n1: the boxes of the cover
whose smallest `reflective` lies below unit_float(n1).  The record is packed array "level1_mirror"; the slab intervals are float32 with
single-rounding FMAs, as the kernel's."""
import ctypes as C

import numpy as np

import level1_restatement as R
import level1_stretch_restatement as S
from kernel_restatements import mt_accepts

f32 = np.float32
PANELS, REST, NW = 12, 4, 8
MIRROR = np.dtype({"names": ["n_panels", "n_rest", "n_w", "thr2", "d2lo", "d2hi", "a0", "m0", "rmin", "w", "rest", "panel"],
                   "formats": ["<i4", "<i4", "<i4", "<f4", "<f4", "<f4", "<f4", "<f4", ("<f4", 8), ("<f4", (NW, 4)), ("<f4", (REST, 8)), ("<f4", (PANELS, 16))],
                   "offsets": [0, 4, 8, 12, 16, 20, 24, 28, 32, 64, 192, 320], "itemsize": 1088})


def mirror(sqt, holder):
    """The Level1Mirror record of holder.scene through sq_scene_pack, or None where the packer wrote none (no cover)."""
    L, h = sqt.lib(), C.c_void_p()
    sqt._native.check(L.sq_scene_pack(C.byref(holder.scene), C.byref(h)))
    try:
        data, n = C.c_void_p(), C.c_size_t()
        assert L.sq_packed_array(h, b"level1_mirror", C.byref(data), C.byref(n)) == 0
        if n.value == 0:
            return None
        assert n.value == MIRROR.itemsize, n.value
        return np.frombuffer(C.string_at(data, n.value), MIRROR)[0]
    finally:
        L.sq_packed_free(h)


def mirror_cannot_reach(M, p0, d1, un1, why=None):
    """The kernel's geometric half of condition (5); every comparison as the kernel writes it (a NaN keeps the sample).
    why = a dict: it receives, per row, which of the four tests keep the sample -- "dd" (|d1|^2 outside its limits), "rest" (a rest box),
    "floor" (a mirrored determinant below the floor), "panel" (a panel whose image can be reached) -- and "tail", the number of panel
    entries beyond n_panels the kernel evaluates with its last group of three."""
    n = len(p0)
    if M is None or int(M["n_panels"]) == 0:
        return np.zeros(n, bool)
    by = {k: np.zeros(n, bool) for k in ("dd", "rest", "floor", "panel")}
    n_read = 3 * ((int(M["n_panels"]) + 2) // 3)                            # the kernel takes them three at a time
    with np.errstate(all="ignore"):
        dd = R.dot32(d1, d1)
        by["dd"] = ~((dd >= M["d2lo"]) & (dd <= M["d2hi"]))
        for j in range(REST):
            tmin, tmax = S.slab_interval(M["rest"][j][:6], p0, d1)
            by["rest"] |= (M["rest"][j][6] >= un1) & ~((tmax <= 0) | (tmin >= tmax))
        floor2 = M["thr2"] * dd
        for k in range(int(M["n_w"])):
            a = R.dot32(d1, np.broadcast_to(M["w"][k][:3], d1.shape))
            by["floor"] |= ~(a * a >= floor2)
        for j in range(n_read):
            b = M["panel"][j]
            pmin, pmax = S.slab_interval(b[0:6], p0, d1)
            imin, imax = S.slab_interval(b[6:12], p0, d1)
            cannot = (pmax < pmin) | (pmax <= -b[12]) | (imax < imin) | (imax < pmin)
            by["panel"] |= (b[13] >= un1) & ~cannot
    if why is not None:
        why.update(by, tail=n_read - int(M["n_panels"]))
    return ~(by["dd"] | by["rest"] | by["floor"] | by["panel"])


def stretch_misses_cover(V, M, p0, d1, nd, lo, hi, m, lim, why=None):
    """Condition (4) restricted to the boxes of the cover whose smallest `reflective` is below lim (per row).  why = a dict: it
    receives the two alternatives per row, "empty" (no stretch) and "may_end" (ray 1 may end in a box, at a point of the stretch)."""
    ta, tb = S.stretch(p0, d1, nd, lo, hi, m)
    empty = ta > tb
    with np.errstate(all="ignore"):
        ta32 = np.where(ta > 1e-30, (ta * (1.0 - 2.0 ** -20)).astype(f32), f32(0))
        tb32 = (tb * (1.0 + 2.0 ** -20)).astype(f32)
    may_end = np.zeros(len(p0), bool)
    for j in range(8):
        tmin, tmax = S.slab_interval(V["box"][j], p0, d1)
        with np.errstate(all="ignore"):
            tlo = (tmin - V["r"][j] * np.abs(tmin)) - V["c"][j]
            thi = (tmax + V["r"][j] * np.abs(tmax)) + V["c"][j]
            may_end |= (np.fmax(tlo, ta32) <= np.fmin(thi, tb32)) & (M["rmin"][j] < lim)
    if why is not None:
        why.update(empty=empty, may_end=may_end)
    return empty | ~may_end


def culled(T, V, M, em, p0, d1, un1, nd, why=None):
    """(culled by (1)-(3), by (4) alone, by (5) alone) for scattered first-bounce rays; the three masks are disjoint.
    why = a dict: it receives "four" (level1_stretch_restatement.culled's report), "mirror" = (rows mirror_cannot_reach judged, its
    report) and "four_under_five" = (rows, stretch_misses_cover's report), each only where that test ran."""
    four = {}
    old, new4 = S.culled(T, V, em, p0, d1, un1, nd, why=four)
    if why is not None:
        why["four"] = four
    new5 = np.zeros(len(p0), bool)
    if not T["on"] or V is None or M is None:
        return old, new4, new5
    c1 = np.ones(len(p0), bool)
    for v0, v1, v2 in em:
        acc, _ = mt_accepts(p0, d1, np.broadcast_to(v0, p0.shape), np.broadcast_to(v1, p0.shape), np.broadcast_to(v2, p0.shape))
        c1 &= ~acc
    nn = R.dot32(nd, nd)
    amin, m = R.ray2_margin(T, em, nd)
    cand = R.ray_in_limits(T, p0, d1) & c1 & ~R.condition2(T, p0, d1, un1) & (nn >= T["d2min"]) & (nn <= T["d2max"])
    sel = np.flatnonzero(cand)
    if len(sel):
        by = {}
        cand[sel] = mirror_cannot_reach(M, p0[sel], d1[sel], un1[sel], why=by)
        if why is not None and by:
            why["mirror"] = (sel, by)
    new5 = cand & np.isinf(amin)
    sel = np.flatnonzero(cand & np.isfinite(amin))
    if len(sel):
        by = {}
        half = R.halfplane_misses_box(p0[sel], d1[sel], nd[sel], T["em_lo"], T["em_hi"], m[sel])
        new5[sel] = half | stretch_misses_cover(V, M, p0[sel], d1[sel], nd[sel], T["em_lo"], T["em_hi"], m[sel], un1[sel], why=by)
        if why is not None:
            by["half"] = half
            why["four_under_five"] = (sel, by)
    assert not (new5 & (old | new4)).any()
    return old, new4, new5


def frame_prediction(sqt, T, V, M, ob, flat, cam, spp, w, h, why=None):
    """(first-bounce rays, masks culled by (1)-(3), by (4) alone, by (5) alone) of a frame; why: as `culled` fills it."""
    fb = R.frame_first_bounces(ob, flat, cam, spp, w, h)
    nd = R.random_vectors(fb["n1"], fb["n2"])
    return (fb,) + culled(T, V, M, R.emitters_of(flat), fb["p0"], fb["d1"], R.unit_float(fb["n1"]), nd, why=why)


def quad(origin, ex, ey):
    """The two triangles of the parallelogram origin + [0, 1] ex + [0, 1] ey, as 2 x 3 x 3 float32."""
    o, ex, ey = (np.asarray(a, np.float64) for a in (origin, ex, ey))
    return np.array([[o, o + ex, o + ex + ey], [o, o + ex + ey, o + ey]]).astype(f32)


def mirror_soup(seed, n_emit, quads, values=(0.0, 0.3, 0.7), **kw):
    """level1_restatement.soup with every random triangle diffuse and planar mirrors added: quads = [(2 x 3 x 3 triangles, index into
    `values`)] overwrite the first non-emissive triangles.  Returns (tris, mats, oracle triangle records)."""
    import pyoracle as O
    tris, mats, _ = R.soup(seed, n_emit, reflective=values, **kw)
    lamp = len(values)
    tris["mat"][tris["mat"] != lamp] = 0
    free = iter(np.flatnonzero(tris["mat"] == 0)[1:])                    # (the first shares an edge with an emitter: soup)
    for q, vi in quads:
        for t in q:
            i = next(free)
            tris["v0"][i], tris["v1"][i], tris["v2"][i], tris["mat"][i] = t[0], t[1], t[2], vi
    ot = np.zeros(len(tris), O.TRI_DTYPE)
    ot["a"], ot["b"], ot["c"] = tris["v0"], tris["v1"], tris["v2"]
    for f in ("reflective", "surf", "emissive", "emit"):
        ot[f] = mats[f][tris["mat"]]
    return tris, mats, ot


# Two soups with mirrors (tests/test_level1_mirror.py, tests/test_gpu_level1_mirror.py): axis-aligned quads of two `reflective` values
# around a clustered emitter group, and one tilted mirror plane of two quads.  (seed, emitters, quads, camera, soup arguments)
def axis_soup():
    q = [(quad((-2.5, -1.5, -1.5), (0, 3, 0), (0, 0, 3)), 1), (quad((-1.5, -2.5, -1.5), (3, 0, 0), (0, 0, 3)), 2),
         (quad((-1.5, -1.5, 2.5), (3, 0, 0), (0, 3, 0)), 1), (quad((2.5, -1.5, -1.5), (0, 3, 0), (0, 0, 3)), 2)]
    return mirror_soup(61, 2, q, cluster=(1.2, 1.2, -1.2), emitter_size=0.6), b"0.1 0.2 0.3\n0.3 0.2 0.1\n"


def tilted_soup():
    ex, ey = np.array([2.4, 0.3, -0.5]), np.array([0.2, 2.2, 0.9])
    o = np.array([-1.4, -1.2, 2.0])
    q = [(quad(o, ex, ey / 2), 2), (quad(o + ey / 2, ex, ey / 2), 2)]
    return mirror_soup(62, 1, q, cluster=(1.0, -1.0, -1.2), emitter_size=0.8), b"0.2 0.1 -0.4\n1.2 0.1 0.3\n"
