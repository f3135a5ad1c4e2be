"""The ways a sample slot can end: on an absorbing primary hit, on a first bounce that misses, on a first
bounce that hits an absorbing surface, on a hit from which ray 2 can reach no emitter, after a traced ray 2 that hits or misses,
and through the pixel's mirror ray.  Only the last two still carry a ray when sq_accumulate runs; the others leave the triangle
of ray 1 (or -1) and sq_accumulate evaluates their radiance.  Every call form that shares these kernels must give, bit for bit,
the oracle's left folds of r and r * r, its avg and its tonemap.

Two random soups (scenes.emitter_soup_scene: diffuse, half-mirror, full-mirror and absorbing emissive triangles, empty space all
around) cover the fates between them: with 12 emissive triangles the last-bounce shortcut is on (a ray 2 is traced only when it can
reach an emitter, and then it hits something), with 80 it is off (every ray 2 is traced, and most miss).  What the oracle can
tell apart by value is asserted in test_the_scenes_cover_the_fates; a first bounce that misses, one from which no emitter can be
reached and a traced ray 2 without light all give exactly s0*0 + e0 and are told apart only by the launch plan and the geometry."""
import functools

import numpy as np
import pytest

import render_options as RO
from bitcmp import ibits
from f32_folds import fold, tonemap_image
from masked_calls import buffers, masked, oracle_samples
from scenes import emitter_soup_scene as soup

pytestmark = pytest.mark.gpu
set_options = functools.partial(RO.set_options, table=RO.FRAME)
f32 = np.float32
W, H, N = 24, 20, 8                     # rows, columns, samples
SECOND = b"-6 0.4 -0.3\n0.05 -0.04 0.02\n"


@pytest.fixture(scope="module", params=[12, 80], ids=["shortcut", "every_ray2"])
def world(request, sqt, O):
    bih, ob, cam_p, cam_o = soup(sqt, O, 4, request.param)
    ds = sqt.DeviceScene(bih, 0)
    samples = oracle_samples(ob, cam_o, N, W, H)
    yield {"ds": ds, "ob": ob, "cam_p": cam_p, "cam_o": cam_o, "samples": samples, "n_emit": request.param}
    ds.close()


def check_moments(O, world, bounds, **opts):
    """A masked call with second moments per range of `bounds`: sums, sums2, avg and rgb against the oracle's folds after each."""
    ds = world["ds"]
    rng_mb = opts.pop("rng_table_mb", None)
    set_options(ds, **opts)
    if rng_mb is not None:
        ds.set_option("rng_table_mb", rng_mb)
    try:
        B = buffers(W, H)
        s = q = None
        for a, b in zip(bounds, bounds[1:]):
            masked(ds, world["cam_p"], N, W, H, a, b, B, np.ones((W, H), np.uint8))
            s, q = fold(world["samples"], a, b, s, q)
            assert np.array_equal(ibits(B["sums"]), ibits(s)), ("sums", b)
            assert np.array_equal(ibits(B["sums2"]), ibits(q)), ("sums2", b)
            want_avg = f32(1) / f32(b) * s
            assert np.array_equal(ibits(B["avg"]), ibits(want_avg)), ("avg", b)
            assert np.array_equal(B["rgb"].cpu().numpy(), tonemap_image(O, want_avg)), ("rgb", b)
    finally:
        set_options(ds)
        if rng_mb is not None:
            ds.set_option("rng_table_mb", 24576)


def test_the_scenes_cover_the_fates(O, world):
    ob, cam_o, samples = world["ob"], world["cam_o"], world["samples"]
    ds = world["ds"]
    ds.render_rows(world["cam_p"], N, W, H)
    assert ds.last_plan()["n_emitters"] == (12 if world["n_emit"] == 12 else -1)      # the shortcut is on / off (more than 64 emitters)
    tris = ob.flatten()
    hit = [[ob.intersect(*O.make_ray(W, H, y, x, cam_o)) for x in range(H)] for y in range(W)]
    tri0 = np.array([[h.tri if h.hit else -1 for h in row] for row in hit])
    live = tri0 >= 0
    surf0, emit0, refl0 = tris["surf"][tri0], (tris["emissive"][:, None] * tris["emit"])[tri0], tris["reflective"][tri0]
    absorbing = live & (surf0 == 0).all(-1)
    assert (~live).any() and absorbing.any()
    assert (refl0[live] == 1).any() and (refl0[live] == 0.5).any() and (live & (refl0 == 0) & ~absorbing).any()   # all, some, no samples mirror
    # absorbing primary hit: every sample is s0*0 + e0
    assert (samples[:, absorbing] == (surf0 * f32(0) + emit0)[absorbing]).all()
    lit = tris[(tris["emissive"] != 0)][0]
    e = lit["emissive"] * lit["emit"]
    scatter = live & ~absorbing
    r = samples[:, scatter]                                                            # [k, pixels, 3]
    s0 = surf0[scatter]
    dark = (r == 0).all(-1)                                                             # a miss, a dead end or a ray 2 without light
    level1 = (r == s0 * (f32(0) * f32(0) + e) + f32(0)).all(-1) & ~dark               # ray 1 hits an emitter: s0 * (0*0 + e) + 0
    assert dark.any() and level1.any()
    level2 = np.zeros_like(dark)
    for s1 in np.unique(tris["surf"][(tris["surf"] != 0).any(-1)], axis=0):            # ray 2 hits an emitter: s0 * (s1 * (0*0 + e) + 0) + 0
        level2 |= (r == s0 * (s1 * e + f32(0)) + f32(0)).all(-1) & ~dark
    assert level2.any()
    assert (dark | level1 | level2).all()                                               # no other value in a three-level path


@pytest.mark.parametrize("opts", [{}, {"rng_table_mb": 0}, {"slots": W * H * 2}, {"slots": W * H * 2, "rng_table_mb": 0},
                                  {"overlap": 1}, {"overlap": 2}, {"overlap": 1, "slots": W * H * 2}, {"overlap": 2, "slots": W * H * 4},
                                  {"resident": 0}, {"primary_pooled": 1}],
                         ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()) or "defaults")
def test_masked_calls_follow_the_oracle_folds(O, world, opts):
    check_moments(O, world, [0, 1, 5, N], **dict(opts))


def test_one_call_and_range_calls(sqt, O, world):
    import torch
    ds, cam = world["ds"], world["cam_p"]
    s, _ = fold(world["samples"], 0, N)
    want_avg = f32(1) / f32(N) * s
    for slots in (512 << 20, W * H * 3):
        set_options(ds, slots=slots)
        try:
            avg, rgb = ds.render_rows(cam, N, W, H)
            sums = torch.empty((W, H, 3), dtype=torch.float32, device="cuda")
            ds.render_rows_range(cam, N, W, H, 0, 3, sums)
            avg2, rgb2 = ds.render_rows_range(cam, N, W, H, 3, N, sums)
            torch.cuda.synchronize()
            for a, r in ((avg, rgb), (avg2, rgb2)):
                assert np.array_equal(ibits(a), ibits(want_avg)) and np.array_equal(r.cpu().numpy(), tonemap_image(O, want_avg))
            assert np.array_equal(ibits(sums), ibits(s))
        finally:
            set_options(ds)


def test_views(sqt, O, world):
    import torch
    ds = world["ds"]
    cams = [world["cam_p"], sqt.camera_from_text(SECOND)]
    want = [world["samples"], oracle_samples(world["ob"], O.camera_from_text(SECOND), N, W, H)]
    for slots in (512 << 20, 2 * W * H * 2):
        set_options(ds, slots=slots)
        try:
            sums = torch.empty((2, W, H, 3), dtype=torch.float32, device="cuda")
            ds.render_views(cams, N, W, H, k_begin=0, k_end=3, sums=sums)
            avg, rgb = ds.render_views(cams, N, W, H, k_begin=3, k_end=N, sums=sums)
            torch.cuda.synchronize()
            for i in range(2):
                s, _ = fold(want[i], 0, N)
                assert np.array_equal(ibits(sums[i]), ibits(s)), i
                assert np.array_equal(ibits(avg[i]), ibits(f32(1) / f32(N) * s)), i
                assert np.array_equal(rgb[i].cpu().numpy(), tonemap_image(O, f32(1) / f32(N) * s)), i
        finally:
            set_options(ds)


def test_callers_rays(sqt, O, world):
    import torch
    ds = world["ds"]
    o, d = ds.camera_rays(world["cam_p"], W, H)
    seeds = sqt.frame_seeds(N, W, H)
    s, _ = fold(world["samples"], 0, N)
    for slots in (512 << 20, W * H * 2):
        set_options(ds, slots=slots)
        try:
            part = ds.raytrace(o, d, seeds=seeds, samples=N, k_range=(0, 5))
            got = ds.raytrace(o, d, seeds=seeds, samples=N, k_range=(5, N), sums=part.sum, want_rgb=True)
            torch.cuda.synchronize()
            assert np.array_equal(ibits(got.sum), ibits(s))
            assert np.array_equal(ibits(got.avg), ibits(f32(1) / f32(N) * s))
            assert np.array_equal(got.rgb.cpu().numpy(), tonemap_image(O, f32(1) / f32(N) * s))
        finally:
            set_options(ds)
