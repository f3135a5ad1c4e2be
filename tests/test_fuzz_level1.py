"""The inputs of tests/test_gpu_fuzz_level1.py, judged without a GPU, on the pytest slice of tests/fuzz_level1.py: the 200 seeds
3000 .. 3199.  On every scene of the slice whose record turns level-1 culling on, the lemma is searched for counter-examples against
the oracle; every sample of every slice frame that a condition culls has the oracle's radiance of a first-bounce miss; the three
packed records keep their invariants; and the slice holds enough of everything the kernel's level1_culled branches on, counted from
the restatements and the packer alone, so that the GPU slice cannot pass vacuously."""
import collections

import numpy as np
import pytest

import fuzz_level1 as FL
import level1_mirror_restatement as M5
import level1_rays as LR
import level1_restatement as R
import level1_stretch_restatement as S

SEEDS = range(3000, 3200)
f32 = np.float32


@pytest.fixture(scope="module")
def table(sqt, O):
    """One case per seed with its records, its first view and `why`: which test decided inside conditions (4) and (5)."""
    out = []
    for seed in SEEDS:
        c = FL.case(seed)
        c.why = {}
        FL.records(c)
        c.t = FL.view(c, why=c.why)
        out.append(c)
    return out


def test_no_culled_ray_of_any_scene_with_level_1_on_reaches_an_emitter(table, O):
    """The counter-example search of tests/test_level1_mirror.py (tests/level1_rays.py, search) with 2 000 rays of each family -- ends
    on mirrors, mirrored at emitter edges, at the determinant floor, uniform -- on every scene of the slice with level-1 on: every ray
    condition (5) culls, and the first 100 of each family that conditions (1)-(4) cull, with the assertions of that test."""
    total = collections.Counter()
    scenes = 0
    for c in table:
        if not c.plan_on:
            continue
        T, _, V, M = FL.records(c)
        ob = FL.oracle(c)
        got = LR.search(np.random.default_rng([c.seed, 5]), FL.describe(c), c.ot, ob, c.flat, T, V, M, n=2000, kept_checked=100, others_checked=100)
        total.update(got)
        scenes += 1
    print(f"{scenes} scenes, {total['rays']} rays: {total['new5']} culled by (5) alone, {total['panel_hits']} of them end on a triangle that mirrors; "
          f"{total['kept_accepted']} kept rays whose mirrored ray 2 an emitter accepts; {total['floor_kept']} rays at the determinant floor kept")
    assert scenes >= 150 and total["panel_hits"] >= 200 and total["kept_accepted"] >= 20 and total["floor_kept"] > 0, total


def test_culled_samples_of_every_frame_have_the_radiance_of_a_first_bounce_miss(table, O):
    """End to end against the oracle: every sample of every slice frame that any condition culls has, from sqo_sample_radiance, the
    bits of s0.surf * 0 + s0.emit (tests/test_level1_mirror.py checks the same on scene.obj)."""
    zero = np.zeros(3, f32)
    n = 0
    for c in table:
        t, ob = c.t, FL.oracle(c)
        for i in np.flatnonzero(t.masks.any(0)):
            y, x, k = int(t.fb["y"][i]), int(t.fb["x"][i]), int(t.fb["k"][i])
            o, d = (np.asarray(a, f32) for a in O.make_ray(c.w, c.h, y, x, t.cam))
            s0 = c.flat[ob.intersect(o, d).tri]
            want = ((s0["surf"] * zero).astype(f32) + (f32(s0["emissive"]) * s0["emit"]).astype(f32)).astype(f32)
            got = np.asarray(ob.sample_radiance(t.cam, c.spp, c.w, c.h, y, x, k), f32)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (FL.describe(c), y, x, k, got, want, t.masks[:, i])
            n += 1
    print(f"{n} culled samples in {len(table)} frames")
    assert n >= 2000


def test_the_records_keep_their_invariants_on_every_scene(table):
    """Byte sizes 200 / 272 / 1088; every non-emissive triangle in a panel of its value or a rest box wherever there are panels; the
    entries beyond a count repeat the first; and past a limit (13 planar groups, 9 W vectors) no panel and no cull by (5)."""
    for c in table:
        T, s, V, M = FL.records(c)
        what = FL.describe(c)
        assert T.nbytes == 200 and (V is None or V.nbytes == 272) and (M is None or M.nbytes == 1088), what
        assert (V is not None) == bool(s["level1_on"]), what
        if V is not None:
            assert all(np.array_equal(V["box"][j], V["box"][0]) and V["r"][j] == V["r"][0] and V["c"][j] == V["c"][0]
                       for j in range(max(int(V["n"]), 1), 8)), what
        if M is None:
            continue
        assert 0 <= M["n_panels"] <= M5.PANELS and 0 <= M["n_rest"] <= M5.REST and 0 <= M["n_w"] <= M5.NW, what
        if M["n_panels"] > 0:
            assert len(LR.uncovered(M, c.ot)) == 0, what
            for f, n in (("panel", "n_panels"), ("w", "n_w"), ("rest", "n_rest")):
                assert all(np.array_equal(M[f][j], M[f][0]) for j in range(max(int(M[n]), 1), len(M[f]))), (what, f)
        else:
            assert not c.t.masks[2].any(), what
        for edge, count, n in (("groups12", "n_panels", 12), ("w8", "n_w", 8)):
            assert c.edge != edge or (M["n_panels"] > 0 and M[count] == n), what
        if c.edge in ("groups13", "w9"):
            assert M["n_panels"] == 0 and not c.t.masks[2].any(), what


def test_a_camera_that_looks_away_gives_empty_first_bounces_and_empty_masks(sqt, O):
    """A frame without a first-bounce ray: frame_first_bounces returns empty arrays of the usual dtypes and ranks, and the three
    frame_prediction functions empty masks."""
    (tris, mats, ot), _ = M5.axis_soup()
    bih = sqt.BIH(sqt.Mesh.from_arrays(tris, mats))
    T, _ = R.tables(sqt, bih)
    V, M = S.cover(sqt, bih), M5.mirror(sqt, bih)
    ob = O.BIH(ot)
    flat = ob.flatten()
    cam = O.camera_from_text(FL.away_camera(np.random.default_rng(1), 60.0))
    assert not any(ob.intersect(*O.make_ray(6, 5, y, x, cam)).hit for y in range(6) for x in range(5))
    fb = R.frame_first_bounces(ob, flat, cam, 2, 6, 5)
    assert {k: (v.dtype, v.shape) for k, v in fb.items()} == {"y": (np.int64, (0,)), "x": (np.int64, (0,)), "k": (np.int64, (0,)), "p0": (f32, (0, 3)),
                                                              "d1": (f32, (0, 3)), "n1": (np.uint32, (0,)), "n2": (np.uint32, (0,))}
    for got in (R.frame_prediction(sqt, T, ob, flat, cam, 2, 6, 5), S.frame_prediction(sqt, T, V, ob, flat, cam, 2, 6, 5),
                M5.frame_prediction(sqt, T, V, M, ob, flat, cam, 2, 6, 5)):
        assert all(m.dtype == bool and m.shape == (0,) for m in got[1:])


# ---- what the slice covers ---------------------------------------------------------------------------------------------------
def sole(by, name):
    """Rows of mirror_cannot_reach's report that `name` alone keeps: without that test the kernel would cull them."""
    others = np.zeros(len(by[name]), bool)
    for k in ("dd", "rest", "floor", "panel"):
        if k != name:
            others |= by[k]
    return by[name] & ~others


def reason_counts(table):
    n = collections.Counter()
    for c in table:
        if "mirror" in c.why:
            _, by = c.why["mirror"]
            for k in ("dd", "rest", "floor", "panel"):
                n[k] += int(sole(by, k).sum())
            n["tail"] += len(by["dd"]) if by["tail"] else 0
        four = c.why.get("four", {})
        if "rows" in four:
            n["empty"] += int(four["empty"].sum())
            n["not_may_end"] += int((~four["empty"] & ~four["may_end"]).sum())
    return n


SCENES = (
    ("level-1 on", lambda c: c.plan_on, 150),
    ("n_panels > 0", lambda c: FL.records(c)[3] is not None and FL.records(c)[3]["n_panels"] > 0, 100),
)
FRAMES = (
    ("a cull by (1)-(3)", lambda c: c.t.masks[0].any(), 40),
    ("a cull by (4) alone", lambda c: c.t.masks[1].any(), 25),
    ("a cull by (5) alone", lambda c: c.t.masks[2].any(), 60),
    ("no first-bounce ray, or level-1 off", lambda c: len(c.t.fb["k"]) == 0 or not c.plan_on, 10),
) + tuple((f"edge scene {e}", lambda c, e=e: c.edge == e, 2) for e in FL.EDGES)


@pytest.mark.parametrize("what, fact, least", SCENES + FRAMES, ids=[c[0] for c in SCENES + FRAMES])
def test_the_slice_covers(table, what, fact, least):
    count = sum(1 for c in table if fact(c))
    print(f"seeds {SEEDS[0]}..{SEEDS[-1]} with {what}: {count} (at least {least} asked)")
    assert count >= least, f"{what}: {count} seeds, {least} asked"


def test_every_scale_and_both_rotation_states_have_frames_that_condition_5_culls_in(table):
    with5 = [c for c in table if c.t.masks[2].any()]
    assert {c.scale for c in with5 if c.family == "room"} >= set(FL.ROOM_SCALES) and {c.rotated for c in with5} == {False, True}


REASONS = ("rest", "floor", "panel", "tail", "empty", "not_may_end")


@pytest.mark.parametrize("reason", REASONS)
def test_each_test_inside_conditions_4_and_5_decides_for_at_least_ten_first_bounce_rays(table, reason):
    """Inside mirror_cannot_reach: a rest box, the determinant floor, and a panel whose image is reachable each keep, alone, at least 10
    first-bounce rays of the slice (a kernel without that test would count them in slot 30); a panel entry of the padded tail is
    evaluated for at least 10; and inside (4) both alternatives, the empty stretch and the stretch no box of the cover meets, cull 10."""
    n = reason_counts(table)
    print(dict(n))
    assert n[reason] >= 10, dict(n)


def test_no_first_bounce_ray_can_have_a_squared_length_outside_the_limits_of_condition_5(table):
    """The fourth way mirror_cannot_reach keeps a sample, |d1|^2 outside [d2lo, d2hi] = [1.01 d2min, 0.99 d2max], cannot decide for a
    ray a frame produces, whatever the generator: d1 is +-randomVector(n1, n2), a unit vector up to float32 rounding, and the limits lie
    a factor away from 1.  So instead of a floor of 10 such rays: there is none, and this is why."""
    for c in table:
        if "mirror" in c.why:
            sel, by = c.why["mirror"]
            M = FL.records(c)[3]
            dd = R.dot32(c.t.fb["d1"][sel], c.t.fb["d1"][sel])
            assert not by["dd"].any() and (np.abs(dd - 1) < 1e-5).all() and M["d2lo"] < 0.9 and M["d2hi"] > 1.1, FL.describe(c)
