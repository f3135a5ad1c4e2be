"""Rays made to probe condition (5) of level-1 culling, and the counter-example search that walks them through the oracle
(tests/test_level1_mirror.py on three placed scenes, tests/test_fuzz_level1.py on the random ones of tests/fuzz_level1.py).

Belongs here: a family of first-bounce rays aimed at where the condition could be wrong -- ends on mirrors, mirror images of emitter
edges, directions at the determinant floor --, and what the oracle does with a ray 1 once it is given.  Needs no GPU."""
import numpy as np

import level1_mirror_restatement as M5
from depth_restatement import cross, dot
from kernel_restatements import mt_accepts

f32 = np.float32


def emissive_of(ot):
    return np.array([(f32(t["emissive"]) * t["emit"].astype(f32)).astype(f32).view(np.uint32).any() for t in ot], bool)


def holds(box, ot, sel):
    """Per selected triangle: are its three vertices inside box (lo.xyz, hi.xyz)?"""
    return np.all([((ot[f][sel] >= box[:3]) & (ot[f][sel] <= box[3:6])).all(1) for f in ("a", "b", "c")], 0)


def uncovered(M, ot):
    """The non-emissive triangles that lie neither in a panel of their own `reflective` value nor in a rest box that answers for it."""
    dark = np.flatnonzero(~emissive_of(ot))
    ok = np.zeros(len(dark), bool)
    val = ot["reflective"][dark].astype(f32)
    for j in range(int(M["n_panels"])):
        ok |= (val == M["panel"][j][13]) & holds(M["panel"][j][:6], ot, dark)
    for j in range(int(M["n_rest"])):
        ok |= (val <= M["rest"][j][6]) & holds(M["rest"][j][:6], ot, dark)
    return dark[~ok]


def mirror_dir(d, t):
    """reflectRay of the oracle (src/Lib.hs:176-181) in float32, as tests/depth_restatement.py walks it."""
    nrm = cross((t["b"] + -t["a"]).astype(f32), (t["c"] + -t["a"]).astype(f32))
    with np.errstate(all="ignore"):
        dn = (nrm / f32(np.sqrt(dot(nrm, nrm)))).astype(f32)
        return (d + -(f32(f32(2) * dot(dn, d)) * dn).astype(f32)).astype(f32)


def unit(v):
    return v / np.maximum(np.linalg.norm(v, axis=1), 1e-300)[:, None]


def points_on(rng, ot, k):
    """A point of each triangle k: inside it, on an edge or on a corner."""
    a, b, c = (ot[f][k].astype(np.float64) for f in ("a", "b", "c"))
    w = rng.dirichlet([1, 1, 1], len(k))
    kind = rng.integers(0, 3, len(k))
    w[kind == 1, 2] = 0; w[kind == 2, 1:] = 0
    w /= w.sum(1)[:, None]
    return w[:, :1] * a + w[:, 1:2] * b + w[:, 2:] * c


def normals(ot, k):
    n = np.cross(ot["b"][k].astype(np.float64) - ot["a"][k], ot["c"][k].astype(np.float64) - ot["a"][k])
    return unit(n)


def rays_ending_on_mirrors(rng, ot, mirrors, n, omax):
    """Ray 1 through a point of a mirroring triangle -- inside, on an edge, on a corner --, any direction."""
    k = rng.choice(mirrors, n)
    p1 = points_on(rng, ot, k)
    d1 = unit(rng.normal(0, 1, (n, 3))).astype(f32)
    t = (10.0 ** rng.uniform(-3, np.log10(0.4 * omax), n))[:, None]
    return (p1 - t * d1).astype(f32), d1


def rays_mirrored_at_emitter_edges(rng, ot, mirrors, em, n, omax):
    """Ray 1 whose mirror image in the plane of a mirroring triangle, taken from a point of it, passes just inside or outside an edge or
    corner of an emitter."""
    k = rng.choice(mirrors, n)
    p1, nh = points_on(rng, ot, k), normals(ot, k)
    e = np.array([[v.astype(np.float64) for v in t] for t in em])[rng.integers(0, len(em), n)]
    ek = rng.integers(0, 3, n)
    va, vb = e[np.arange(n), ek], e[np.arange(n), (ek + 1) % 3]
    tgt = va + (rng.random(n) * (rng.random(n) < 0.7))[:, None] * (vb - va)
    out = unit(tgt - e.mean(1))
    tgt = tgt + (10.0 ** rng.uniform(-9, -1, n) * rng.choice([-1.0, 1.0], n))[:, None] * out
    d2 = unit(tgt - p1)
    d1 = (d2 - 2 * (d2 * nh).sum(1)[:, None] * nh).astype(f32)
    t = (10.0 ** rng.uniform(-3, np.log10(0.4 * omax), n))[:, None]
    return (p1 - t * d1).astype(f32), d1


def rays_at_the_determinant_floor(rng, ot, mirrors, M, n, omax):
    """Ray 1 through a point of a mirroring triangle whose |d1 . W| / |d1| lies within a few parts in a thousand of the floor, either side."""
    k = rng.choice(mirrors, n)
    p1 = points_on(rng, ot, k)
    W = M["w"][rng.integers(0, int(M["n_w"]), n), :3].astype(np.float64)
    wl = np.linalg.norm(W, axis=1)
    c = np.sqrt(float(M["thr2"])) / wl * (1 + rng.uniform(-3e-3, 3e-3, n)) * rng.choice([-1.0, 1.0], n)
    side = rng.normal(0, 1, (n, 3)); side = unit(side - (side * W).sum(1)[:, None] * W / (wl * wl)[:, None])
    d1 = (c[:, None] * W / wl[:, None] + np.sqrt(np.maximum(1 - c * c, 0))[:, None] * side).astype(f32)
    t = (10.0 ** rng.uniform(-3, np.log10(0.4 * omax), n))[:, None]
    return (p1 - t * d1).astype(f32), d1


def uniform_rays(rng, n, vmax):
    return (rng.uniform(-vmax, vmax, (n, 3)) / np.sqrt(3)).astype(f32), unit(rng.normal(0, 1, (n, 3))).astype(f32)


def families(rng, ot, mirrors, em, M, n, omax):
    """(name, (p0, d1)) of the four families, n rays each, in the order the search has always drawn them.  A family that needs a
    mirroring triangle, an emitter or a W vector is left out where the scene has none."""
    if len(mirrors):
        yield "ends", rays_ending_on_mirrors(rng, ot, mirrors, n, omax)
        if em:
            yield "edges", rays_mirrored_at_emitter_edges(rng, ot, mirrors, em, n, omax)
        if M is not None and int(M["n_panels"]) and int(M["n_w"]):
            yield "floor", rays_at_the_determinant_floor(rng, ot, mirrors, M, n, omax)
    yield "uniform", uniform_rays(rng, n, omax / 2)


def search(rng, name, ot, ob, flat, T, V, M, n, kept_checked=500, others_checked=0):
    """The counter-example search of one scene.  For every ray 1 condition (5) culls no emitter accepts ray 1, the oracle's traversal
    returns a miss or a non-emissive triangle, and no emitter's mollerTrumbore accepts the ray 2 the oracle forms from the hit point it
    computes: the mirrored direction where the triangle mirrors under n1, +-nd where it scatters.  The same is asserted of the first
    `others_checked` rays of each family that conditions (1)-(3) or (4) cull.  Of the rays no condition culls, the first `kept_checked`
    of each family are walked as well, to count those the mirrored ray 2 of which an emitter does accept.
    Returns {"new5", "panel_hits", "kept_accepted", "floor_kept", "rays"}."""
    import level1_restatement as R
    em = R.emitters_of(ot)
    emissive = emissive_of(flat)
    mirrors = np.flatnonzero(~emissive_of(ot) & (ot["reflective"] > 0))
    top = float(ot["reflective"][mirrors].max()) if len(mirrors) else 1.0
    omax = float(np.sqrt(T["o2max"]))
    E = [np.array([t[k] for t in em], f32).reshape(-1, 3) for k in range(3)]

    def accepted(o, d):
        """The number of emitters whose mollerTrumbore accepts the ray (o, d)."""
        if not em:
            return 0
        return int(mt_accepts(np.broadcast_to(o, E[0].shape), np.broadcast_to(d, E[0].shape), *E)[0].sum())

    out = dict.fromkeys(("new5", "panel_hits", "kept_accepted", "floor_kept", "rays"), 0)
    for which, (p0, d1) in list(families(rng, ot, mirrors, em, M, n, omax)):      # every family is drawn before the first un1
        un1 = (rng.random(n) * top * 1.2).astype(f32)
        nd = unit(rng.normal(0, 1, (n, 3))).astype(f32)
        old, new4, new5 = M5.culled(T, V, M, em, p0, d1, un1, nd)
        out["new5"] += int(new5.sum())
        out["rays"] += n
        kept = np.flatnonzero(~old & ~new4 & ~new5)
        if which == "floor":
            out["floor_kept"] += len(kept)
        gone = old | new4 | new5
        for i in np.concatenate([np.flatnonzero(new5), np.flatnonzero(old | new4)[:others_checked], kept[:kept_checked]]):
            if gone[i]:
                assert not accepted(p0[i], d1[i]), (name, which, int(i))             # condition (1)
            hit = ob.intersect(p0[i], d1[i])
            if not hit.hit:
                continue
            t = flat[hit.tri]
            if gone[i]:
                assert not emissive[hit.tri], (name, which, int(i))
            if emissive[hit.tri]:
                continue
            p1 = np.array([hit.point.x, hit.point.y, hit.point.z], f32)
            mirrors_here = not (t["reflective"] < un1[i])
            dirs = [mirror_dir(d1[i], t)] if mirrors_here else [nd[i], -nd[i]]
            out["panel_hits"] += int(new5[i] and mirrors_here)
            for d2 in dirs:
                acc = accepted(p1, d2)
                if gone[i]:
                    assert not acc, (name, which, int(i), p0[i], d1[i], un1[i], nd[i], bool(new5[i]))
                else:
                    out["kept_accepted"] += acc * int(mirrors_here)
    return out
