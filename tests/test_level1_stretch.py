"""Condition (4) of level-1 culling (squigly-trace_amd/csrc/sq_pack_level1.h, build_level1 and level1_cover): the cover the packer
builds, and the lemma's extension searched for counter-examples on the CPU.

Claim: a scattered first-bounce ray (p0, d1) that conditions (1) and (2) pass and whose stretch -- the part of it from which the
line along randomVector(n1, n2) reaches the emitters' grown box -- is empty, or ends in no box of the cover, belongs to a sample
whose radiance is level0_radiance of its pixel: whatever the traversal returns for ray 1, no emitter accepts ray 2 from there.
tests/level1_stretch_restatement.py states the condition as the kernel evaluates it."""
import importlib
import os

import numpy as np
import pytest

import level1_restatement as R
import level1_stretch_restatement as S
from kernel_restatements import mt_accepts
from level1_restatement import soup

sqt = importlib.import_module("squigly-trace_amd")
N = importlib.import_module("squigly-trace_amd._native")
DATA = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data")
f32 = np.float32


def bih_of(tris, mats):
    return sqt.BIH(sqt.Mesh.from_arrays(tris, mats))


def boxes_holding(V, pts):
    """Per point: does some box of the cover hold it?"""
    b = V["box"][:int(V["n"])]
    return ((pts[:, None, :] >= b[None, :, :3]) & (pts[:, None, :] <= b[None, :, 3:])).all(2).any(1)


def test_cover_holds_every_non_emissive_triangle():
    import pyoracle as O
    scene = sqt.BIH(sqt.Mesh.from_obj(os.path.join(DATA, "scene.obj"), DATA))
    V = S.cover(sqt, scene)
    ot = O.tris_from_obj(os.path.join(DATA, "scene.obj"), DATA)
    dark = np.array([not (f32(t["emissive"]) * t["emit"].astype(f32)).astype(f32).view(np.uint32).any() for t in ot])
    assert 1 < V["n"] <= 8                                               # a room: walls and panels get boxes of their own
    for f in ("a", "b", "c"):
        assert boxes_holding(V, ot[f][dark].astype(f32)).all()
    # strictly inside: every box is grown beyond its triangles
    lo, hi = V["box"][:int(V["n"]), :3], V["box"][:int(V["n"]), 3:]
    assert (hi > lo).all()
    print("scene.obj cover:", V["n"], "boxes, growth of the room's box", float((hi.max(0) - lo.min(0) - (ot["a"][dark].max(0) - ot["a"][dark].min(0))).max()))

    assert (V["r"][:int(V["n"])] > 0).all() and (V["r"] <= 0.126).all() and (V["c"][:int(V["n"])] > 0).all()   # r_T <= 1/8 by P <= 29

    # a soup has no thin triangles: the octants of its box; more than 8 groups are merged down to 8; level1 off: no record
    tris, mats, ot = soup(31, 2)
    V1 = S.cover(sqt, bih_of(tris, mats))
    assert 1 <= V1["n"] <= 8
    for f in ("r", "c", "box"):                                          # the entries beyond n repeat the first: the kernel reads all eight
        assert all(np.array_equal(V1[f][j], V1[f][0]) for j in range(int(V1["n"]), 8))
    dark = tris["mat"] != len(mats) - 1
    for f in ("v0", "v1", "v2"):
        assert boxes_holding(V1, tris[f][dark]).all()
    rng = np.random.default_rng(3)
    for k in range(40):                                                  # panels at 20 heights, two triangles each
        z = f32(-1.0 + 0.1 * (k // 2))
        tris["v0"][k], tris["v1"][k], tris["v2"][k] = (f32([*rng.uniform(-1, 1, 2), z]) for _ in range(3))
    V2 = S.cover(sqt, bih_of(tris, mats))
    assert V2["n"] == 8
    dark = tris["mat"] != len(mats) - 1
    for f in ("v0", "v1", "v2"):
        assert boxes_holding(V2, tris[f][dark]).all()
    assert S.cover(sqt, bih_of(*soup(7, 65)[:2])) is None


def aimed_rays(rng, ot, em, n, omax):
    """Adversarial (p0, d1, nd): p1 on a non-emissive triangle -- inside it, on an edge or on a corner, so that it lies on or next to a
    face of a cover box -- and ray 2 aimed from p1 at a point just outside or inside an edge or corner of an emitter, so that the
    end of ray 1 sits at an end of the stretch; ray 1 is drawn THROUGH p1."""
    dark = np.flatnonzero([not (f32(t["emissive"]) * t["emit"].astype(f32)).astype(f32).view(np.uint32).any() for t in ot])
    k = rng.choice(dark, n)
    a, b, c = (ot[f][k].astype(np.float64) for f in ("a", "b", "c"))
    w = rng.dirichlet([1, 1, 1], n)
    kind = rng.integers(0, 3, n)
    w[kind == 1, 2] = 0; w[kind == 2, 1:] = 0                            # an edge, a corner
    w /= w.sum(1)[:, None]
    p1 = w[:, :1] * a + w[:, 1:2] * b + w[:, 2:] * c
    j = rng.integers(0, len(em), n)
    e = np.array([[v.astype(np.float64) for v in t] for t in em])[j]     # n x 3 x 3
    lam = rng.random(n)
    ek = rng.integers(0, 3, n)
    va, vb = e[np.arange(n), ek], e[np.arange(n), (ek + 1) % 3]
    tgt = va + (lam * (rng.random(n) < 0.7))[:, None] * (vb - va)        # on an edge, or the corner itself
    out = tgt - e.mean(1)
    out /= np.maximum(np.linalg.norm(out, axis=1), 1e-300)[:, None]
    tgt = tgt + (10.0 ** rng.uniform(-9, -1, n) * rng.choice([-1.0, 1.0], n))[:, None] * out
    nd = tgt - p1
    nd = (nd / np.maximum(np.linalg.norm(nd, axis=1), 1e-300)[:, None] * rng.choice([-1.0, 1.0], n)[:, None]).astype(f32)
    d1 = rng.normal(0, 1, (n, 3)); d1 /= np.linalg.norm(d1, axis=1)[:, None]
    d1 = d1.astype(f32)
    t = (10.0 ** rng.uniform(-3, np.log10(0.4 * omax), n)).astype(f32)
    p0 = (p1 - t[:, None] * d1).astype(f32)
    return p0, d1, nd


def uniform_rays(rng, n, vmax):
    p0 = (rng.uniform(-vmax, vmax, (n, 3)) / np.sqrt(3)).astype(f32)
    d1 = rng.normal(0, 1, (n, 3)); d1 /= np.linalg.norm(d1, axis=1)[:, None]
    nd = rng.normal(0, 1, (n, 3)); nd /= np.linalg.norm(nd, axis=1)[:, None]
    return p0, d1.astype(f32), nd.astype(f32)


SCENES = {**{k: R.NAMED_SOUPS[k] for k in ("one", "two_clustered", "many_clustered")}, "scene.obj": None}


@pytest.mark.parametrize("name", list(SCENES))
def test_no_sample_condition_4_culls_reaches_an_emitter(name):
    """Counter-example search.  For every ray 1 the new condition culls, the oracle's traversal returns a miss or a non-emissive
    triangle, and from the hit point it computes no emitter's mollerTrumbore accepts nd or -nd.  Both sides of the search must be
    populated: rays the condition culls, and rays it keeps whose ray 2 IS accepted (the aimed ones are made for that)."""
    import pyoracle as O
    rng = np.random.default_rng(20261019)
    if name == "scene.obj":
        ot = O.tris_from_obj(os.path.join(DATA, "scene.obj"), DATA)
        bih = sqt.BIH(sqt.Mesh.from_obj(os.path.join(DATA, "scene.obj"), DATA))
    else:
        t, m, ot = SCENES[name]()
        bih = bih_of(t, m)
    T, s = R.tables(sqt, bih)
    V = S.cover(sqt, bih)
    assert s["level1_on"] == 1 and V is not None
    em = R.emitters_of(ot)
    ob = O.BIH(ot)
    flat = ob.flatten()
    emissive = np.array([(f32(t["emissive"]) * t["emit"].astype(f32)).astype(f32).view(np.uint32).any() for t in flat])
    omax = float(np.sqrt(T["o2max"]))
    n_new = n_old = n_new_hits = n_kept_accepted = n_stretch_only = 0
    for p0, d1, nd in (aimed_rays(rng, ot, em, 20000, omax), uniform_rays(rng, 20000, omax / 2)):
        un1 = rng.random(len(p0)).astype(f32)
        old, new = S.culled(T, V, em, p0, d1, un1, nd)
        _, new_a = S.culled(T, V, em, p0, d1, un1, nd, use_cover=False)
        assert not (old & new).any() and not (new_a & ~new).any()        # a superset of the old rule, and the cover only adds
        n_old += int(old.sum()); n_new += int(new.sum()); n_stretch_only += int(new_a.sum())
        kept = np.flatnonzero(~old & ~new)
        for i in np.concatenate([np.flatnonzero(new), kept[:400]]):
            hit = ob.intersect(p0[i], d1[i])
            if not hit.hit:
                continue
            if new[i]:
                assert not emissive[hit.tri], (name, i)                  # condition (1)
                n_new_hits += 1
            p1 = np.array([[hit.point.x, hit.point.y, hit.point.z]], f32)
            for v0, v1, v2 in em:
                for sign in (f32(1), f32(-1)):
                    acc, _ = mt_accepts(p1, sign * nd[i:i + 1], v0[None], v1[None], v2[None])
                    if new[i]:
                        assert not acc[0], (name, int(i), p0[i], d1[i], nd[i])
                    else:
                        n_kept_accepted += int(acc[0])
    print(f"{name}: {n_old} culled by (1)-(3), {n_new} by (4) alone ({n_stretch_only} by the stretch without the cover), {n_new_hits} of those "
          f"hit a triangle; {n_kept_accepted} kept rays whose ray 2 an emitter accepts")
    assert n_new > 200 and n_new_hits > 50 and n_kept_accepted > 20, (n_new, n_new_hits, n_kept_accepted)


def test_culled_samples_of_a_frame_have_the_radiance_of_a_first_bounce_miss(oracle_scene):
    """End to end against the oracle, scene.obj at 40 x 72 @ 3: every sample the old or the new condition culls has, from
    sqo_sample_radiance, the bits of s0.surf * 0 + s0.emit; and the frame is not vacuous: condition (4) culls at least 5 % of its
    first-bounce rays beyond conditions (1)-(3)."""
    w, h, spp = 40, 72, 3
    ob, cam, _ = oracle_scene
    flat = ob.flatten()
    scene = sqt.BIH(sqt.Mesh.from_obj(os.path.join(DATA, "scene.obj"), DATA))
    T, _ = R.tables(sqt, scene)
    V = S.cover(sqt, scene)
    fb, old, new = S.frame_prediction(sqt, T, V, ob, flat, cam, spp, w, h)
    _, old_a, new_a = S.frame_prediction(sqt, T, V, ob, flat, cam, spp, w, h, use_cover=False)
    print(f"{w}x{h} @ {spp}: of {len(old)} first-bounce rays {int(old.sum())} culled by (1)-(3) ({old.mean():.3f}), {int(new.sum())} more by (4) "
          f"({new.mean():.3f}); the stretch without the cover: {int(new_a.sum())} ({new_a.mean():.3f})")
    assert np.array_equal(old, old_a) and not (old & new).any() and not (new_a & ~new).any()
    assert new.mean() >= 0.05, new.mean()
    zero = np.zeros(3, f32)
    for i in np.flatnonzero(old | new):
        y, x, k = int(fb["y"][i]), int(fb["x"][i]), int(fb["k"][i])
        o, d = (np.asarray(a, f32) for a in __import__("pyoracle").make_ray(w, h, y, x, cam))
        t = flat[ob.intersect(o, d).tri]
        want = ((t["surf"] * zero).astype(f32) + (f32(t["emissive"]) * t["emit"]).astype(f32)).astype(f32)
        got = np.asarray(ob.sample_radiance(cam, spp, w, h, y, x, k), f32)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (y, x, k, got, want, bool(new[i]))
