"""sq_temporal_accumulate_moving_device's contract (include/squigly_temporal.h) restated in numpy float32, one operation per line in
the header's order, on top of tests/temporal_restatement.py.

Belongs here: `move_back` (a pixel's point and normal through its object's B), `window_bounds` (the clamp's lo and hi), `accumulate`
and `chain` with flags, and `tables`, the seeded object and transform tables the CPU and the GPU tests share.  With no objects and no
clamp `accumulate` is temporal_restatement.accumulate, which tests/test_moving.py asserts bit for bit."""
import numpy as np

import temporal_restatement as R

f = np.float32
BLENDED, CLAMPED, MOVED = 1, 2, 4


def move_back(tri, normal, point, objects, back):
    """(P', n', moved): objects int32 [n_tris], back float32 [n_objects, 12]; None, None = nothing moves.  An index outside its
    table is never read through."""
    nrm, pnt = np.asarray(normal, f), np.asarray(point, f)
    tri = np.asarray(tri, np.int32)
    if objects is None:
        return pnt, nrm, np.zeros(tri.shape, bool)
    objects, back = np.asarray(objects, np.int32).reshape(-1), np.asarray(back, f).reshape(-1, 12)
    n_tris, n_objects = len(objects), len(back)
    known = (tri >= 0) & (tri < n_tris)
    o = np.where(known, objects[np.clip(tri, 0, n_tris - 1)], -1).astype(np.int64)
    moved = known & (o >= 0) & (o < n_objects)
    B = back[np.clip(o, 0, n_objects - 1)]
    with np.errstate(all="ignore"):
        Pm = np.stack([((B[..., 4 * i] * pnt[..., 0] + B[..., 4 * i + 1] * pnt[..., 1]) + B[..., 4 * i + 2] * pnt[..., 2]) + B[..., 4 * i + 3]
                       for i in range(3)], -1)
        nm = np.stack([(B[..., 4 * i] * nrm[..., 0] + B[..., 4 * i + 1] * nrm[..., 1]) + B[..., 4 * i + 2] * nrm[..., 2] for i in range(3)], -1)
    return np.where(moved[..., None], Pm, pnt).astype(f), np.where(moved[..., None], nm, nrm).astype(f), moved


def window_bounds(color, tri, radius, k):
    """(lo, hi, sd) [rows, cols, 3] of the clamp's window; meaningful where tri >= 0 (the centre counts, n >= 1)."""
    c, tri = np.asarray(color, f), np.asarray(tri, np.int32)
    rows, cols = tri.shape
    k = f(k)
    n = np.zeros((rows, cols), f)
    s, s2 = np.zeros((rows, cols, 3), f), np.zeros((rows, cols, 3), f)
    yy, xx = np.mgrid[0:rows, 0:cols]
    with np.errstate(all="ignore"):
        for j in range(-radius, radius + 1):
            for i in range(-radius, radius + 1):
                qy, qx = yy + j, xx + i
                inside = (qy >= 0) & (qy < rows) & (qx >= 0) & (qx < cols)
                gy, gx = np.clip(qy, 0, rows - 1), np.clip(qx, 0, cols - 1)
                counts = inside & (tri[gy, gx] >= 0)
                Cq = c[gy, gx]
                n = np.where(counts, n + f(1), n)
                s = np.where(counts[..., None], s + Cq, s)
                s2 = np.where(counts[..., None], s2 + Cq * Cq, s2)
        mu = s / n[..., None]
        vr = s2 / n[..., None] - mu * mu
        vr = np.where(vr > 0, vr, f(0))
        sd = np.sqrt(vr)
        ks = k * sd
        return (mu - ks).astype(f), (mu + ks).astype(f), sd.astype(f)


def accumulate(color, var, tri, normal, point, prev_cam, prev, alpha=None, objects=None, back=None, clamp=None, alpha_min=0.1,
               max_history=32, sigma_p=0.0353, cos_n=0.9):
    """sq_temporal_accumulate_moving_device: dict(color, var, len, flags, block).  clamp = (radius, k) or None."""
    c, v = np.array(color, f), np.array(var, f)
    tri = np.asarray(tri, np.int32)
    nrm, pnt = np.asarray(normal, f), np.asarray(point, f)
    rows, cols = tri.shape
    out_c, out_v, out_len = c.copy(), v.copy(), np.ones((rows, cols), np.int32)
    flags = np.zeros((rows, cols), np.uint8)
    if prev is not None:
        alpha_min, sigma_p, cos_n = f(alpha_min), f(sigma_p), f(cos_n)
        with np.errstate(all="ignore"):
            Pm, nm, moved = move_back(tri, nrm, pnt, objects, back)
            ok, fx, fy = R.project(prev_cam, rows, cols, Pm)
            ok &= tri >= 0
            fx, fy = np.where(ok, fx, f(0)), np.where(ok, fy, f(0))
            x0, y0 = np.floor(fx), np.floor(fy)
            tx, ty = fx - x0, fy - y0
            ix, iy = x0.astype(np.int64), y0.astype(np.int64)
            sw = np.zeros((rows, cols), f)
            sc = np.zeros((rows, cols, 3), f)
            sv = np.zeros((rows, cols), f)
            m = np.full((rows, cols), 0x7fffffff, np.int64)
            for j in (0, 1):
                for i in (0, 1):
                    qy, qx = iy + j, ix + i
                    inside = ok & (qy >= 0) & (qy < rows) & (qx >= 0) & (qx < cols)
                    gy, gx = np.clip(qy, 0, rows - 1), np.clip(qx, 0, cols - 1)
                    acc = inside & (prev["tri"][gy, gx] >= 0)
                    nq, Pq, Cq, Vq, Lq = prev["normal"][gy, gx], prev["point"][gy, gx], prev["color"][gy, gx], prev["var"][gy, gx], prev["len"][gy, gx]
                    bw = (tx if i else f(1) - tx) * (ty if j else f(1) - ty)
                    dn = (nm[..., 0] * nq[..., 0] + nm[..., 1] * nq[..., 1]) + nm[..., 2] * nq[..., 2]
                    acc &= dn >= cos_n
                    d = Pq - Pm
                    pd = (nm[..., 0] * d[..., 0] + nm[..., 1] * d[..., 1]) + nm[..., 2] * d[..., 2]
                    acc &= np.abs(pd) <= sigma_p
                    sw = np.where(acc, sw + bw, sw)
                    sc = np.where(acc[..., None], sc + bw[..., None] * Cq, sc)
                    sv = np.where(acc, sv + bw * Vq, sv)
                    m = np.where(acc, np.minimum(m, Lq.astype(np.int64)), m)
            blend = sw > 0
            hc = sc / sw[..., None]
            hv = sv / sw
            clamped = np.zeros((rows, cols), bool)
            if clamp is not None:
                lo, hi, _ = window_bounds(c, tri, int(clamp[0]), clamp[1])
                below = hc < lo
                hc = np.where(below, lo, hc)
                above = hc > hi
                hc = np.where(above, hi, hc)
                clamped = (below | above).any(-1)
            m1 = np.where(blend, m + 1, 1)
            a = f(1) / m1.astype(f)
            a = np.where(a < alpha_min, alpha_min, a)
            if alpha is not None:
                al = np.asarray(alpha, f)
                a = np.where(a < al, al, a)
            bc = hc + a[..., None] * (c - hc)
            om = f(1) - a
            bv = (om * om) * hv + (a * a) * v
            out_c = np.where(blend[..., None], bc, c).astype(f)
            out_v = np.where(blend, bv, v).astype(f)
            out_len = np.where(blend, np.minimum(m1, int(max_history)), 1).astype(np.int32)
            flags = (BLENDED * blend + CLAMPED * (blend & clamped) + MOVED * moved).astype(np.uint8)
    block = dict(color=out_c, var=out_v, len=out_len, tri=tri.copy(), normal=nrm.copy(), point=pnt.copy())
    return dict(color=out_c, var=out_v, len=out_len, flags=flags, block=block)


def chain(frames, cams, alphas=None, objects=None, backs=None, clamp=None, **params):
    """temporal_restatement.chain under geometry that moves: objects[f] is frame f's triangle table (or one table for all), backs[f]
    the move from frame f - 1's geometry to frame f's (backs[0] is not read)."""
    outs, prev, prev_cam = [], None, None
    for i, (frame, cam) in enumerate(zip(frames, cams)):
        obj = None if objects is None else objects[i] if isinstance(objects, (list, tuple)) else objects
        r = accumulate(*frame, prev_cam, prev, alpha=None if alphas is None else alphas[i], objects=obj if backs is not None else None,
                       back=None if backs is None else backs[i], clamp=clamp, **params)
        outs.append(r)
        prev, prev_cam = r["block"], cam
    return outs


def rigid(angle, axis, t):
    """A row-major 3 x 4 [R | t]: a rotation by `angle` about the unit `axis` (Rodrigues, float64), then the translation t."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    Rm = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
    return np.concatenate([Rm, np.asarray(t, np.float64).reshape(3, 1)], 1)


IDENTITY_ROW = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], f)


def tables(n_tris, seed):
    """(objects int32 [n_tris], back float32 [5, 12]) for the synthetic frames (triangles 10 and 20): triangle 10, the far wall, is
    object 1 (a small real rotation plus translation: some taps still pass the stops), triangle 20 object 0 (identity); the other
    entries (scatter_triangles puts them into a frame) take every kind of index -- -1, n_objects - 1, n_objects, large positive, large negative.  Rows 2 and 3 are NaN and
    infinite, row 4 (n_objects - 1) a sideways slide."""
    kinds = np.array([-1, 0, 1, 2, 3, 4, 5, 2 ** 31 - 1, -2 ** 31, 1 << 20, -7], np.int64)
    objects = kinds[(np.arange(n_tris) + seed) % len(kinds)].astype(np.int32)          # every kind, from 11 triangles up
    if n_tris > R.FAR_TRI:
        objects[R.FAR_TRI] = 1
    if n_tris > R.NEAR_TRI:
        objects[R.NEAR_TRI] = 0
    back = np.stack([IDENTITY_ROW, rigid(0.004, (0.2, 1, 0.3), (0.001, 0.03, -0.02)).reshape(12).astype(f), np.full(12, np.nan, f),
                     np.array([1, 0, 0, np.inf, 0, 1, 0, 0, 0, 0, 1, -np.inf], f), rigid(0, (0, 0, 1), (0, 0.05, 0)).reshape(12).astype(f)])
    return objects, back


def scatter_triangles(tri, n_tris, seed, share=0.3):
    """Gives about `share` of the hit pixels of `tri` (in place) a seeded triangle id in [0, n_tris): the frame then looks up every
    entry of a table, not only the two planes'."""
    rng = np.random.default_rng(seed)
    pick = (tri >= 0) & (rng.random(tri.shape) < share)
    tri[pick] = rng.integers(0, n_tris, int(pick.sum()), dtype=np.int32)
    return tri
