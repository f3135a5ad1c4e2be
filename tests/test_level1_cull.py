"""Level-1 culling (squigly-trace_amd/csrc/sq_pack_level1.h, build_level1): the lemma behind it, searched for counter-examples on the CPU.

Claim: a scattered first-bounce ray (p0, d1) that passes the three conditions (tests/level1_restatement.py states them as the
kernel does) belongs to a sample whose radiance is level0_radiance of its pixel: no emitter accepts ray 1, nothing ray 1 can hit
mirrors, and from no point of ray 1 does the reference's fp32 mollerTrumbore accept an emitter along +-randomVector(n1, n2).
"""
import importlib
import os

import numpy as np
import pytest

import level1_restatement as R
from kernel_restatements import grazing_rays as _grazing_rays, mt_accepts, slab_passes
from level1_restatement import soup

sqt = importlib.import_module("squigly-trace_amd")
N = importlib.import_module("squigly-trace_amd._native")
DATA = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data")
f32 = np.float32


def bih_of(tris, mats):
    return sqt.BIH(sqt.Mesh.from_arrays(tris, mats))


def test_flag_and_tables_on_both_sides_of_their_switches():
    scene = sqt.BIH(sqt.Mesh.from_obj(os.path.join(DATA, "scene.obj"), DATA))
    T, s = R.tables(sqt, scene)
    assert s == {"level1_on": 1, "level1_zero": 1, "n_emitters": 2, "nonneg_materials": 1}
    assert T["n_classes"] == 3 and list(T["class_val"][:3]) == [f32(0.0), f32(0.2), f32(1.0)]          # data/scene.sq
    assert np.all(T["class_box"][0][:3] <= T["class_box"][1][:3]) and np.all(T["class_box"][1][:3] <= T["class_box"][2][:3])   # nested
    assert np.all(T["class_box"][0][3:] >= T["class_box"][1][3:]) and np.all(T["class_box"][1][3:] >= T["class_box"][2][3:])
    assert list(T["em_lo"]) == [-1.0, -1.0, float(f32(2.05))] and list(T["em_hi"]) == [1.0, 1.0, float(f32(2.05))]
    assert 0 < T["em_add"] < 1e-4 and 0 < T["em_rho"] < 4

    # 64 emitters: on; 65: the emitter list, and with it the reduction, is off
    for n_emit, on in ((64, 1), (65, 0)):
        T, s = R.tables(sqt, bih_of(*soup(7, n_emit)[:2]))
        assert (s["level1_on"], s["n_emitters"]) == (on, 64 if on else -1)

    # a -0 emission: the triangle is an emitter (its bits are not +0) and the material is not >= +0: off; +0: on
    for emit, on in (((0.0, 0.0, 0.0), 1), ((-0.0, 0.0, 0.0), 0)):
        tris, mats, _ = soup(8, 3)
        mats["emissive"][1] = 2.0
        mats["emit"][1] = emit
        T, s = R.tables(sqt, bih_of(tris, mats))
        assert s["level1_on"] == on and s["level1_zero"] == 1, (emit, s)
        assert s["n_emitters"] == (3 if on else 3 + int((tris["mat"] == 1).sum()))

    # an emitter beyond the lemma's reach (P = |e1| |e2| 1.25 > 29): off; a non-emitter beyond it: off as well (p1 is unbounded)
    for which in ("emitter", "other"):
        tris, mats, _ = soup(9, 2)
        k = np.flatnonzero((tris["mat"] == len(mats) - 1) == (which == "emitter"))[0]
        tris["v1"][k] = tris["v0"][k] + f32([6, 0, 0]); tris["v2"][k] = tris["v0"][k] + f32([0, 6, 0])
        assert R.tables(sqt, bih_of(tris, mats))[1]["level1_on"] == 0
    tris, mats, _ = soup(9, 2)
    assert R.tables(sqt, bih_of(tris, mats))[1]["level1_on"] == 1

    # no mirror class: one value, 0, which only a zero draw reaches; more values than classes: the lowest merge upward
    T, _ = R.tables(sqt, bih_of(*soup(10, 2, reflective=(0.0,))[:2]))
    assert T["n_classes"] == 1 and T["class_val"][0] == 0
    p0 = np.zeros((2, 3), f32); d1 = np.tile(f32([0.6, 0.6, 0.52]), (2, 1))
    assert list(R.condition2(T, p0, d1, f32([0.0, 1e-9]))) == [False, True]
    T6, _ = R.tables(sqt, bih_of(*soup(10, 2)[:2]))
    assert T6["n_classes"] == 4 and list(T6["class_val"]) == [f32(0.3), f32(0.5), f32(0.8), f32(1.0)]
    Tall, _ = R.tables(sqt, bih_of(*soup(10, 2, reflective=(0.0, 0.0, 0.0, 0.0, 0.0, 0.0))[:2]))
    assert np.array_equal(T6["class_box"][0], Tall["class_box"][0])     # the merged class holds every triangle


def oracle_tris(name):
    import pyoracle as O
    if name == "scene.obj":
        tris = O.tris_from_obj(os.path.join(DATA, "scene.obj"), DATA)
        return sqt.BIH(sqt.Mesh.from_obj(os.path.join(DATA, "scene.obj"), DATA)), tris
    t, m, ot = R.NAMED_SOUPS[name]()
    return bih_of(t, m), ot


@pytest.mark.parametrize("name", ["scene.obj", "soup", "soup_big_emitters"])
def test_no_culled_pair_is_accepted(name):
    """Counter-example search.  Rays (p1, nd) aimed just outside the edges and corners of an emitter with determinants barely above
    eps (tests/test_cull.py), and uniform ones; ray 1 is drawn THROUGH p1, so that p1 = fl(p0 + fl(t d1)) is what the kernels
    compute.  No pair that condition 3 culls may be accepted by mollerTrumbore for nd or -nd, for any emitter; and no ray 1 that
    condition 2 passes may be accepted by a triangle of its class."""
    rng = np.random.default_rng(20261018)
    bih, ot = oracle_tris(name)
    T, s = R.tables(sqt, bih)
    assert s["level1_on"] == 1
    em = R.emitters_of(ot)
    et = np.zeros(len(em), N.TRI_DTYPE)
    et["v0"], et["v1"], et["v2"] = [e[0] for e in em], [e[1] for e in em], [e[2] for e in em]
    # aim at the emitters that own a face of the emitters' box: only next to those can a ray near an emitter leave the box
    allv = np.stack([et["v0"], et["v1"], et["v2"]], 1)
    et = et[np.unique(np.concatenate([allv.min(1).argmin(0), allv.max(1).argmax(0)]))]
    omax = float(np.sqrt(T["o2max"]))
    vmax = omax / 2
    culled_n = accepted_n = 0
    worst = 0.0
    for eps_scale in (0.05, 0.5, 2.0, None):
        n = 80_000
        if eps_scale is None:                                            # uniform: p1 in the scene, nd towards a random point of an emitter
            k = rng.integers(0, len(et), n)
            wgt = rng.dirichlet([1, 1, 1], n)
            tgt = wgt[:, :1] * et["v0"][k] + wgt[:, 1:2] * et["v1"][k] + wgt[:, 2:] * et["v2"][k] + rng.normal(0, 0.3, (n, 3)) * rng.integers(0, 2, (n, 1))
            p1 = rng.uniform(-vmax, vmax, (n, 3)) / np.sqrt(3)
            nd = tgt - p1
            nd /= np.linalg.norm(nd, axis=1)[:, None]
            p1, nd = p1.astype(f32), nd.astype(f32)
        else:
            k, p1, nd = _grazing_rays(rng, et, n, 0.45 * omax, eps_scale)
            nd = (nd / np.linalg.norm(nd.astype(np.float64), axis=1)[:, None]).astype(f32)     # randomVector is a unit vector
        n = len(k)
        # ray 1 through p1: p0 = p1 - t d1, then p1 as the kernels form it
        d1 = rng.normal(0, 1, (n, 3)); d1 /= np.linalg.norm(d1, axis=1)[:, None]
        t = (10.0 ** rng.uniform(-3, 0.5, n)).astype(f32)
        d1 = d1.astype(f32)
        p0 = (p1 - t[:, None] * d1).astype(f32)
        p1 = (p0 + (t[:, None] * d1).astype(f32)).astype(f32)
        ok = R.ray_in_limits(T, p0, d1)
        k, p0, d1, p1, nd = k[ok], p0[ok], d1[ok], p1[ok], nd[ok]
        c3 = R.condition3(T, em, p0, d1, nd)
        culled_n += int(c3.sum())
        amin, m = R.ray2_margin(T, em, nd)
        for j, (v0, v1, v2) in enumerate(em):
            V0, V1, V2 = (np.broadcast_to(x, p1.shape) for x in (v0, v1, v2))
            for sign in (f32(1), f32(-1)):
                acc, a = mt_accepts(p1, sign * nd, V0, V1, V2)
                assert not (acc & c3).any(), (name, j, int((acc & c3).sum()), p0[acc & c3][:2], d1[acc & c3][:2], nd[acc & c3][:2])
                accepted_n += int(acc.sum())
                if acc.any():
                    # how much of the margin do accepted rays use?  Chebyshev distance from the half-line to the emitter's own box,
                    # over the margin granted for the determinant it was accepted with (as tests/test_cull.py measures the leaf margin)
                    o64, d64 = p1[acc].astype(np.float64), (sign * nd[acc]).astype(np.float64)
                    lo, hi = np.minimum(np.minimum(v0, v1), v2).astype(np.float64), np.maximum(np.maximum(v0, v1), v2).astype(np.float64)
                    fdist = lambda tt: np.maximum(np.maximum(lo - (o64 + tt[:, None] * d64), (o64 + tt[:, None] * d64) - hi), 0).max(1)   # noqa: E731
                    lo_t = np.zeros(len(o64)); hi_t = np.full(len(o64), 8 * omax)
                    for _ in range(120):
                        m1 = lo_t + (hi_t - lo_t) / 3; m2 = hi_t - (hi_t - lo_t) / 3
                        left = fdist(m1) <= fdist(m2)
                        hi_t = np.where(left, m2, hi_t); lo_t = np.where(left, lo_t, m1)
                    grant = T["em_rho"] * (1e-4 / np.abs(a[acc]).astype(np.float64)) + T["em_add"]
                    worst = max(worst, float((fdist((lo_t + hi_t) / 2) / grant).max()))
        # condition 2: a ray 1 that passes it is rejected by every triangle that would mirror
        un1 = rng.random(len(p0)).astype(f32)
        c2 = R.condition2(T, p0, d1, un1)
        refl = ot["reflective"]
        for j in rng.choice(np.flatnonzero(refl > 0), min(40, int((refl > 0).sum())), replace=False):
            tri = ot[j]
            acc, _ = mt_accepts(p0, d1, *(np.broadcast_to(tri[f].astype(f32), p0.shape) for f in ("a", "b", "c")))
            assert not (acc & c2 & (refl[j] >= un1)).any(), (name, "class", int(j))
    assert culled_n > 300 and accepted_n > 20_000, (culled_n, accepted_n)      # neither side of the search is empty (rays aimed AT an emitter are rarely culled)
    assert worst < 0.5, worst
    print(f"{name}: {culled_n} culled and {accepted_n} accepted (p1, nd, emitter) pairs, none both; largest (distance to emitter box) / (margin granted) = {worst:.4f}")


def test_grazing_mirror_rays_pass_their_class_box():
    """Rays that graze triangles of scene.obj's mirror mesh and are accepted pass the slab test of every class box that holds them."""
    import pyoracle as O
    rng = np.random.default_rng(5)
    scene = sqt.BIH(sqt.Mesh.from_obj(os.path.join(DATA, "scene.obj"), DATA))
    T, _ = R.tables(sqt, scene)
    ot = O.tris_from_obj(os.path.join(DATA, "scene.obj"), DATA)
    mt = np.zeros(int((ot["reflective"] == 1).sum()), N.TRI_DTYPE)
    for f, g in (("v0", "a"), ("v1", "b"), ("v2", "c")):
        mt[f] = ot[g][ot["reflective"] == 1]
    total = 0
    for eps_scale in (0.05, 0.5, 2.0):
        k, o, d = _grazing_rays(rng, mt, 100_000, 0.999 * float(np.sqrt(T["o2max"])), eps_scale)
        ok = R.ray_in_limits(T, o, d)
        k, o, d = k[ok], o[ok], d[ok]
        acc, _ = mt_accepts(o, d, mt["v0"][k], mt["v1"][k], mt["v2"][k])
        total += int(acc.sum())
        for c in range(3):
            assert slab_passes(np.broadcast_to(T["class_box"][c], (int(acc.sum()), 6)), o[acc], d[acc]).all(), c
    assert total > 10_000, total


@pytest.mark.parametrize("w,h,spp", [(40, 72, 3)])
def test_culled_samples_of_a_frame_have_the_radiance_of_a_first_bounce_miss(oracle_scene, w, h, spp):
    """End to end against the oracle: every sample of the frame that the restatement culls has, from sqo_sample_radiance, the bits
    of s0.surf * 0 + s0.emit; and the culled share is far above the floor the GPU test relies on (one ray 1 in ten)."""
    ob, cam, _ = oracle_scene
    flat = ob.flatten()
    scene = sqt.BIH(sqt.Mesh.from_obj(os.path.join(DATA, "scene.obj"), DATA))
    T, _ = R.tables(sqt, scene)
    fb, c = R.frame_prediction(sqt, T, ob, flat, cam, spp, w, h)
    assert c.mean() > 0.3, c.mean()
    zero = np.zeros(3, f32)
    for i in np.flatnonzero(c):
        y, x, k = int(fb["y"][i]), int(fb["x"][i]), int(fb["k"][i])
        o, d = (np.asarray(a, f32) for a in __import__("pyoracle").make_ray(w, h, y, x, cam))
        t = flat[ob.intersect(o, d).tri]
        want = ((t["surf"] * zero).astype(f32) + (f32(t["emissive"]) * t["emit"]).astype(f32)).astype(f32)
        got = np.asarray(ob.sample_radiance(cam, spp, w, h, y, x, k), f32)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (y, x, k, got, want)
    print(f"{w}x{h} @ {spp}: {int(c.sum())} of {len(c)} first-bounce rays culled ({c.mean():.3f})")
