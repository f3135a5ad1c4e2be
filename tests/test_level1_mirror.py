"""Condition (5) of level-1 culling (squigly-trace_amd/csrc/sq_host.cpp, level1_tables and level1_mirror): the record the packer
builds, and the lemma's mirror extension searched for counter-examples on the CPU.

Claim: a scattered first-bounce ray (p0, d1) that condition (1) passes, that is inside the ray limits and that condition (5) culls
belongs to a sample whose radiance is level0_radiance of its pixel: whatever the traversal returns for ray 1, no emitter accepts the
ray 2 that leaves it -- mirrored where the triangle mirrors under n1, along +-randomVector(n1, n2) where it scatters.
tests/level1_mirror_restatement.py states the condition as the kernel evaluates it."""
import importlib
import os

import numpy as np
import pytest

import level1_mirror_restatement as M5
import level1_restatement as R
import level1_stretch_restatement as S
from depth_restatement import cross, dot
from kernel_restatements import mt_accepts

sqt = importlib.import_module("squigly-trace_amd")
DATA = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data")
f32 = np.float32


def bih_of(tris, mats):
    return sqt.BIH(sqt.Mesh.from_arrays(tris, mats))


def emissive_of(ot):
    return np.array([(f32(t["emissive"]) * t["emit"].astype(f32)).astype(f32).view(np.uint32).any() for t in ot])


def scene_obj():
    import pyoracle as O
    return O.tris_from_obj(os.path.join(DATA, "scene.obj"), DATA), sqt.BIH(sqt.Mesh.from_obj(os.path.join(DATA, "scene.obj"), DATA))


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


def parallel_mirrors(n):
    """A soup with n mirror quads on parallel planes, one emitter."""
    q = [(M5.quad((-1.5, -1.5, -2.0 + 0.3 * k), (3, 0, 0), (0, 3, 0)), 1 + k % 2) for k in range(n)]
    return M5.mirror_soup(63, 1, q, cluster=(1.2, 1.2, 2.6), emitter_size=0.5)


def test_every_mirroring_triangle_lies_in_a_panel_or_a_rest_box_and_the_count_limits_hold():
    ot, scene = scene_obj()
    M = M5.mirror(sqt, scene)
    assert R.tables(sqt, scene)[0].nbytes == 200 and S.cover(sqt, scene).nbytes == 272 and M.nbytes == 1088
    assert (M["n_panels"], M["n_w"]) == (9, 1) and 1 <= M["n_rest"] <= M5.REST  # the room's nine walls; the lamp's two triangles share a plane
    assert len(uncovered(M, ot)) == 0
    assert 0 < M["m0"] < 0.01 and 1e-4 <= M["a0"] < 0.1
    for (tris, mats, ot), _ in (M5.axis_soup(), M5.tilted_soup()):
        M = M5.mirror(sqt, bih_of(tris, mats))
        assert M["n_panels"] > 0 and len(uncovered(M, ot)) == 0
        for f, n in (("panel", "n_panels"), ("w", "n_w"), ("rest", "n_rest")):   # the entries beyond a count repeat the first
            assert all(np.array_equal(M[f][j], M[f][0]) for j in range(int(M[n]), len(M[f])))
    # twelve panels fit, thirteen switch the condition off; so do nine W vectors (one panel, nine emitters in general position) after eight
    rng = np.random.default_rng(5)
    for make, n_ok, count in ((parallel_mirrors, 12, "n_panels"),
                              (lambda n: M5.mirror_soup(64, n, [(M5.quad((-1.5, -1.5, -2.5), (3, 0, 0), (0, 3, 0)), 2)]), 8, "n_w")):
        for n in (n_ok, n_ok + 1):
            tris, mats, ot = make(n)
            bih = bih_of(tris, mats)
            T, s = R.tables(sqt, bih)
            V, M = S.cover(sqt, bih), M5.mirror(sqt, bih)
            assert s["level1_on"] == 1 and M.nbytes == 1088
            p0 = rng.uniform(-1, 1, (4000, 3)).astype(f32)
            d1 = rng.normal(0, 1, (4000, 3)); d1 = (d1 / np.linalg.norm(d1, axis=1)[:, None]).astype(f32)
            nd = rng.normal(0, 1, (4000, 3)); nd = (nd / np.linalg.norm(nd, axis=1)[:, None]).astype(f32)
            un1 = rng.random(4000).astype(f32)
            em = R.emitters_of(ot)
            old, new4, new5 = M5.culled(T, V, M, em, p0, d1, un1, nd)
            old_s, new4_s = S.culled(T, V, em, p0, d1, un1, nd)
            assert np.array_equal(old, old_s) and np.array_equal(new4, new4_s)
            if n == n_ok:
                assert M[count] == n and M["n_panels"] > 0, (count, n)
            else:
                assert M["n_panels"] == 0 and not new5.any(), (count, n)


def mirror_dir(d, t):
    """reflectRay of the oracle (src/Lib.hs:176-181) in float32, as tests/depth_restatement.py walks it."""
    nrm = cross((t["b"] + -t["a"]).astype(f32), (t["c"] + -t["a"]).astype(f32))
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


@pytest.mark.parametrize("name", ["scene.obj", "axis_soup", "tilted_soup"])
def test_no_sample_condition_5_culls_reaches_an_emitter(name):
    """Counter-example search.  For every ray 1 condition (5) culls no emitter accepts ray 1, the oracle's traversal returns a miss or
    a non-emissive triangle, and no emitter's mollerTrumbore accepts the ray 2 the oracle forms from the hit point it computes: the
    mirrored direction where the triangle mirrors under n1, +-nd where it scatters.  Both sides must be populated."""
    import pyoracle as O
    rng = np.random.default_rng(20261020)
    if name == "scene.obj":
        ot, bih = scene_obj()
    else:
        (tris, mats, ot), _ = getattr(M5, name)()
        bih = bih_of(tris, mats)
    T, s = R.tables(sqt, bih)
    V, M = S.cover(sqt, bih), M5.mirror(sqt, bih)
    assert s["level1_on"] == 1 and M["n_panels"] > 0
    em = R.emitters_of(ot)
    ob = O.BIH(ot)
    flat = ob.flatten()
    emissive = emissive_of(flat)
    mirrors = np.flatnonzero(~emissive_of(ot) & (ot["reflective"] > 0))
    top = float(ot["reflective"][mirrors].max())
    omax = float(np.sqrt(T["o2max"]))
    n = 12000
    n_new5 = n_panel_hits = n_kept_accepted = n_floor_kept = 0
    for which, (p0, d1) in (("ends", rays_ending_on_mirrors(rng, ot, mirrors, n, omax)), ("edges", rays_mirrored_at_emitter_edges(rng, ot, mirrors, em, n, omax)),
                            ("floor", rays_at_the_determinant_floor(rng, ot, mirrors, M, n, omax)), ("uniform", uniform_rays(rng, n, omax / 2))):
        un1 = (rng.random(n) * top * 1.2).astype(f32)
        nd = unit(rng.normal(0, 1, (n, 3))).astype(f32)
        old, new4, new5 = M5.culled(T, V, M, em, p0, d1, un1, nd)
        n_new5 += int(new5.sum())
        kept = np.flatnonzero(~old & ~new4 & ~new5)
        if which == "floor":
            n_floor_kept += len(kept)
        for i in np.concatenate([np.flatnonzero(new5), kept[:500]]):
            if new5[i]:
                for v0, v1, v2 in em:                                    # condition (1)
                    assert not mt_accepts(p0[i:i + 1], d1[i:i + 1], v0[None], v1[None], v2[None])[0][0], (name, which, int(i))
            hit = ob.intersect(p0[i], d1[i])
            if not hit.hit:
                continue
            t = flat[hit.tri]
            if new5[i]:
                assert not emissive[hit.tri], (name, which, int(i))
            if emissive[hit.tri]:
                continue
            p1 = np.array([[hit.point.x, hit.point.y, hit.point.z]], f32)
            mirrors_here = not (t["reflective"] < un1[i])
            dirs = [mirror_dir(d1[i], t)] if mirrors_here else [nd[i], -nd[i]]
            n_panel_hits += int(new5[i] and mirrors_here)
            for d2 in dirs:
                for v0, v1, v2 in em:
                    acc, _ = mt_accepts(p1, d2[None], v0[None], v1[None], v2[None])
                    if new5[i]:
                        assert not acc[0], (name, which, int(i), p0[i], d1[i], un1[i], nd[i])
                    else:
                        n_kept_accepted += int(acc[0] and mirrors_here)
    print(f"{name}: {n_new5} culled by (5) alone, {n_panel_hits} of them end on a triangle that mirrors; {n_kept_accepted} kept rays whose mirrored "
          f"ray 2 an emitter accepts; {n_floor_kept} of {n} rays at the determinant floor kept")
    assert n_panel_hits >= 200 and n_kept_accepted >= 20 and 0 < n_floor_kept < n, (n_new5, n_panel_hits, n_kept_accepted, n_floor_kept)


def test_culled_samples_of_a_frame_have_the_radiance_of_a_first_bounce_miss(oracle_scene):
    """End to end against the oracle, scene.obj at 40 x 72 @ 3: every sample any condition culls has, from sqo_sample_radiance, the bits
    of s0.surf * 0 + s0.emit; condition (5) alone culls at least 8 % of the frame's first-bounce rays; and the masks of (1)-(3) and of
    (4) are those of tests/level1_stretch_restatement.py."""
    import pyoracle as O
    w, h, spp = 40, 72, 3
    ob, cam, _ = oracle_scene
    flat = ob.flatten()
    _, scene = scene_obj()
    T, _ = R.tables(sqt, scene)
    V, M = S.cover(sqt, scene), M5.mirror(sqt, scene)
    fb, old, new4, new5 = M5.frame_prediction(sqt, T, V, M, ob, flat, cam, spp, w, h)
    _, old_s, new4_s = S.frame_prediction(sqt, T, V, ob, flat, cam, spp, w, h)
    print(f"{w}x{h} @ {spp}: of {len(old)} first-bounce rays {int(old.sum())} culled by (1)-(3), {int(new4.sum())} more by (4), {int(new5.sum())} more by (5) "
          f"({new5.mean():.3f})")
    assert np.array_equal(old, old_s) and np.array_equal(new4, new4_s)
    assert not (new5 & (old | new4)).any()
    assert new5.mean() >= 0.08, new5.mean()
    zero = np.zeros(3, f32)
    for i in np.flatnonzero(old | new4 | new5):
        y, x, k = int(fb["y"][i]), int(fb["x"][i]), int(fb["k"][i])
        o, d = (np.asarray(a, f32) for a in O.make_ray(w, h, y, x, cam))
        t = flat[ob.intersect(o, d).tri]
        want = ((t["surf"] * zero).astype(f32) + (f32(t["emissive"]) * t["emit"]).astype(f32)).astype(f32)
        got = np.asarray(ob.sample_radiance(cam, spp, w, h, y, x, k), f32)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (y, x, k, got, want, bool(new5[i]))
