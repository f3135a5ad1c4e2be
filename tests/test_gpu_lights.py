"""Caller-given point lights (sq_scene_set_lights, DeviceScene.set_lights): cast frames and raycast queries under any lights are bit
for bit the formula of include/squigly_hip.h, in the per-lane form and in the wavefront form (option "cast_wavefront").

The expected values come from the CPU oracle alone: rays from O.make_ray, hits (hit, tri, point, dist) from O.BIH.intersect, surface
colours from O.BIH.flatten(), and the formula in numpy float32 with the header's parenthesisation (`restate`).  For the reference's
light that restatement is bit-equal to O.BIH.render(..., cast=True) (test_the_reference_light_in_every_spelling checks it)."""
import functools
import itertools

import numpy as np
import pytest

import render_options as RO
import tree_padding as TP
from bitcmp import nan_eq
from lights_restatement import Restatement, as_light, avg_of, fold_cast as fold
from scenes import ROTATED

pytestmark = pytest.mark.gpu
f32 = np.float32
W = H = 24
# the six positions of the fixture; in the multi-light cases every light has an RGB power of its own, so that a permuted or a
# dropped light changes bits
POSITIONS = ((0, 3, -1), (0, 0, 0), (1.5, -2, 0.5), (-2, 1, 2), (0, 0, 4), (100, 100, 100))
POWERS = ((2, 2, 2), (1.5, 0.5, 0.25), (0.25, 2, 1), (3, 0.75, 0.5), (0.5, 1, 4), (50, 80, 20))
SIX = tuple(zip(POSITIONS, POWERS))
THREE = (SIX[1], SIX[2], SIX[5])
# the three forms of a cast computation, and the options that must not change a bit
# (variant 1 stays one lane per ray whatever cast_wavefront says)
FORMS = (("variant1", {"variant": 1, "cast_wavefront": 0}), ("variant1_wavefront_asked", {"variant": 1, "cast_wavefront": 1}),
         ("per_lane", {"variant": 2, "cast_wavefront": 0}), ("wavefront", {"variant": 2, "cast_wavefront": 1}))
BOTH = FORMS[2:]
options = functools.partial(RO.set_options, table=RO.CAST)


@pytest.fixture(scope="module")
def world(sqt, O, oracle_scene, product_scene):
    ob, ocam, _ = oracle_scene
    bih, cam, _ = product_scene
    ds = sqt.DeviceScene(bih, 0)
    yield {"sqt": sqt, "O": O, "ob": ob, "ocam": ocam, "bih": bih, "cam": cam, "ds": ds, "R": Restatement(O, ob)}
    ds.close()


def shard_rows(sqt, w, shard):
    rb, si, ns = shard
    sh = sqt.Shard(w if rb is None else rb, si, ns)
    return [sqt.lib().sq_shard_global_row(j, sh) for j in range(sqt.lib().sq_shard_rows(w, sh))]


def frame_rays(wd, w, h, shard=(None, 0, 1), ocam=None, tag="cam"):
    """(key, rays) of a shard's pixels in local row-major order."""
    ocam = wd["ocam"] if ocam is None else ocam
    ys = shard_rows(wd["sqt"], w, shard)
    return (tag, w, h, shard), [wd["O"].make_ray(w, h, y, x, ocam) for y in ys for x in range(h)]


def expected_frame(wd, lights, spp, w, h, shard=(None, 0, 1), ocam=None, tag="cam"):
    key, rays = frame_rays(wd, w, h, shard, ocam, tag)
    T, lit = wd["R"].radiance(key, rays, lights)
    avg = avg_of(fold(T, 0, spp), spp)
    rgb = np.array([wd["O"].tonemap(tuple(float(v) for v in c)) for c in avg], np.uint8)
    rows = len(shard_rows(wd["sqt"], w, shard))
    return avg.reshape(rows, h, 3), rgb.reshape(rows, h, 3), T.reshape(rows, h, 3), lit


def gpu_frame(wd, spp, w, h, shard=(None, 0, 1), cam=None):
    import torch
    avg, rgb = wd["ds"].render_rows(wd["cam"] if cam is None else cam, spp, w, h, cast=True, shard=shard)
    torch.cuda.synchronize()
    return avg.cpu().numpy(), rgb.cpu().numpy()


def assert_frame(got, want, what):
    assert nan_eq(got[0], want[0]).all(), f"{what}: avg differs from the restatement"
    assert np.array_equal(got[1], want[1]), f"{what}: rgb differs from the restatement"


def assert_lights_matter(lit, lights):
    """Every light of the fixture lights at least 10 of the hit pixels and leaves at least 10 in shadow."""
    for j, li in enumerate(lights):
        assert (lit[:, j] == 1).sum() >= 10 and (lit[:, j] == 0).sum() >= 10, f"light {li}: {(lit[:, j] == 1).sum()} lit, {(lit[:, j] == 0).sum()} shadowed"


def test_the_fixture_is_the_issues(world):
    """361 of the 576 pixels hit, and the lit / shadowed counts of the six positions at power 2."""
    key, rays = frame_rays(world, W, H)
    _, lit = world["R"].radiance(key, rays, [(p, (2, 2, 2)) for p in POSITIONS])
    assert int((lit[:, 0] >= 0).sum()) == 361
    assert [(int((lit[:, j] == 1).sum()), int((lit[:, j] == 0).sum())) for j in range(6)] == [(320, 41), (250, 111), (82, 279), (17, 344), (41, 320), (199, 162)]


ALL_SETTINGS = [(name, {**form, "resident": r, "pool": p, "primary_pooled": pp})
                for (name, form), r, p, pp in itertools.product(FORMS, (1, 0), (1, 0), (0, 1))]


@pytest.mark.parametrize("case", ["one_light_1spp", "one_light_3spp", "six_lights_2spp", "shard_40x72", "three_lights_5x7"])
def test_oracle_parity_in_every_form_and_option(world, case):
    lights, spp, w, h, shard = {
        "one_light_1spp": ((SIX[2],), 1, W, H, (None, 0, 1)), "one_light_3spp": ((SIX[2],), 3, W, H, (None, 0, 1)),
        "six_lights_2spp": (SIX, 2, W, H, (None, 0, 1)), "shard_40x72": ((SIX[1],), 1, 40, 72, (2, 1, 3)),
        "three_lights_5x7": (THREE, 1, 5, 7, (None, 0, 1))}[case]
    ds = world["ds"]
    want = expected_frame(world, lights, spp, w, h, shard)
    if (w, h) == (W, H):
        assert_lights_matter(want[3], lights)
    ds.set_lights(lights)
    assert np.array_equal(ds.lights, np.array([np.concatenate(as_light(li)) for li in lights], f32))
    for name, opts in ALL_SETTINGS:
        options(ds, **opts)
        got = gpu_frame(world, spp, w, h, shard)
        assert_frame(got, want, f"{case} {name} {opts}")
        plan = ds.last_plan()
        wave = opts["variant"] == 2 and opts["cast_wavefront"] == 1
        assert (plan["trace_form"] != "per_pixel") == wave and (plan["primary_form"] != "none") == wave, (name, opts, plan)
        if wave:
            assert plan["primary_form"] == ("pooled" if opts["primary_pooled"] and opts["pool"] else "resident" if opts["resident"] else "per_lane")


def test_the_reference_light_in_every_spelling(world):
    """Unset, reset, set explicitly -- each is O.BIH.render(cast=True), in every form.  And the six-light order with the other five
    at power 0: their terms are +0 (lit: 0 / dl * surf with dl > 0 finite) or +0 (shadowed), so T = c_0 + 0 + ... is c_0 bit for bit
    on every pixel where c_0 is not -0 and no 0 / dl is NaN; on this fixture (finite positive dl everywhere, c_0 >= +0) that is
    every pixel, which the test asserts from the restatement before it relies on it."""
    sqt, ds, ob, ocam = world["sqt"], world["ds"], world["ob"], world["ocam"]
    want_avg, want_rgb, _ = ob.render(ocam, 3, W, H, cast=True)
    mine = expected_frame(world, [sqt.REFERENCE_LIGHT], 3, W, H)
    assert np.array_equal(mine[0].view(np.uint32), want_avg.view(np.uint32)) and np.array_equal(mine[1], want_rgb)
    zeros = [SIX[0]] + [(p, (0, 0, 0)) for p in POSITIONS[1:]]
    with_zeros = expected_frame(world, zeros, 3, W, H)
    same_arithmetic = np.array_equal(with_zeros[0].view(np.uint32), want_avg.view(np.uint32))
    assert same_arithmetic                                        # all 576 pixels of this fixture
    fresh = sqt.DeviceScene(world["bih"], 0)
    try:
        for name, form in FORMS:
            options(fresh, **form)
            a, r = fresh.render_rows(world["cam"], 3, W, H, cast=True)
            assert np.array_equal(a.cpu().numpy().view(np.uint32), want_avg.view(np.uint32)) and np.array_equal(r.cpu().numpy(), want_rgb), f"unset, {name}"
            assert np.array_equal(fresh.lights, np.array([[0, 3, -1, 2, 2, 2]], f32))
    finally:
        fresh.close()
    for spelling, lights in (("reset", None), ("explicit", [sqt.REFERENCE_LIGHT]), ("zeros", zeros)):
        ds.set_lights(THREE)
        ds.set_lights(lights)
        for name, form in FORMS:
            options(ds, **form)
            got = gpu_frame(world, 3, W, H)
            assert np.array_equal(got[0].view(np.uint32), want_avg.view(np.uint32)) and np.array_equal(got[1], want_rgb), f"{spelling}, {name}"


def test_light_batches(world):
    """Five lights, one per batch (five batches) and two per batch (three batches, the last one short): the carry between batches
    keeps the fold.  A workspace only grows and batches are sized by what it holds, so the small-`slots` frames run on a fresh
    scene whose workspace has never been larger, smallest first, and the number of trace launches says how many batches ran."""
    import torch
    sqt, ds = world["sqt"], world["ds"]
    lights = SIX[1:]
    want = expected_frame(world, lights, 2, W, H)
    ds.set_lights(lights)
    options(ds, cast_wavefront=1)
    whole = gpu_frame(world, 2, W, H)
    assert_frame(whole, want, "default slots")
    fresh = sqt.DeviceScene(world["bih"], 0)
    try:
        fresh.set_lights(lights)
        fresh.enable_timing(True)
        for slots, batches in ((W * H, 5), (2 * W * H, 3)):              # growing: one light per batch, then two
            options(fresh, cast_wavefront=1, slots=slots)
            fresh.reset_timing()
            avg, rgb = fresh.render_rows(world["cam"], 2, W, H, cast=True)
            torch.cuda.synchronize()
            got = (avg.cpu().numpy(), rgb.cpu().numpy())
            _, launches, kernel = fresh.kernel_timing()
            assert (launches, kernel) == (batches, "sq_trace_rays"), f"slots {slots}: {launches} launches of {kernel}"
            assert_frame(got, want, f"slots {slots}")
            assert nan_eq(got[0], whole[0]).all() and np.array_equal(got[1], whole[1])
            assert fresh.last_plan()["trace_form"] != "per_pixel"
    finally:
        fresh.close()


@pytest.mark.parametrize("name, form", BOTH)
def test_ranges_and_masks(world, name, form):
    import torch
    ds, cam = world["ds"], world["cam"]
    ds.set_lights(THREE)
    options(ds, **form)
    key, rays = frame_rays(world, W, H)
    T, lit = world["R"].radiance(key, rays, THREE)
    T = T.reshape(W, H, 3)
    hit = (lit[:, 0] >= 0).reshape(W, H)
    dev = torch.device("cuda", 0)
    # ranges [0, 2) [2, 5) against [0, 5) and the restatement
    s_parts = torch.empty((W, H, 3), dtype=torch.float32, device=dev)
    ds.render_rows_range(cam, 5, W, H, 0, 2, s_parts, cast=True)
    a2, r2 = ds.render_rows_range(cam, 5, W, H, 2, 5, s_parts, cast=True)
    s_whole = torch.empty((W, H, 3), dtype=torch.float32, device=dev)
    a1, r1 = ds.render_rows_range(cam, 5, W, H, 0, 5, s_whole, cast=True)
    torch.cuda.synchronize()
    want_sum = fold(T, 0, 5)
    assert nan_eq(s_whole.cpu().numpy(), want_sum).all() and nan_eq(s_parts.cpu().numpy(), want_sum).all()
    assert nan_eq(a1.cpu().numpy(), avg_of(want_sum, 5)).all() and nan_eq(a2.cpu().numpy(), a1.cpu().numpy()).all()
    assert np.array_equal(r1.cpu().numpy(), r2.cpu().numpy())
    # a checkerboard mask: live pixels get sum, sum2, count, avg and rgb; dead ones keep their sentinels
    mask_np = ((np.arange(W)[:, None] + np.arange(H)[None, :]) % 2).astype(np.uint8)
    mask = torch.from_numpy(mask_np).to(dev)
    sums = torch.full((W, H, 3), 7.5, dtype=torch.float32, device=dev)
    sums2 = torch.full((W, H, 3), 7.5, dtype=torch.float32, device=dev)
    counts = torch.full((W, H), -3, dtype=torch.int32, device=dev)
    avg = torch.full((W, H, 3), 7.5, dtype=torch.float32, device=dev)
    rgb = torch.full((W, H, 3), 9, dtype=torch.uint8, device=dev)
    ds.render_rows_masked(cam, 3, W, H, 0, 2, sums, mask=mask, sums2=sums2, counts=counts, cast=True, out_avg=avg, out_rgb=rgb)
    torch.cuda.synchronize()
    live = mask_np != 0
    want_s = fold(T, 0, 2)
    with np.errstate(all="ignore"):
        want_q = fold((T * T).astype(f32), 0, 2)
    want_a = avg_of(want_s, 2)
    want_rgb = np.array([world["O"].tonemap(tuple(float(v) for v in c)) for c in want_a.reshape(-1, 3)], np.uint8).reshape(W, H, 3)
    got = {k: t.cpu().numpy() for k, t in (("s", sums), ("q", sums2), ("c", counts), ("a", avg), ("r", rgb))}
    assert nan_eq(got["s"][live], want_s[live]).all() and nan_eq(got["q"][live], want_q[live]).all()
    assert (got["c"][live] == 2).all()
    assert nan_eq(got["a"][live], want_a[live]).all() and np.array_equal(got["r"][live], want_rgb[live])
    miss = live & ~hit
    assert miss.sum() >= 10 and (got["a"][miss].view(np.uint32) == 0).all() and (got["r"][miss] == 0).all() and (got["s"][miss].view(np.uint32) == 0).all()
    dead = ~live
    assert (got["s"][dead] == 7.5).all() and (got["q"][dead] == 7.5).all() and (got["c"][dead] == -3).all()
    assert (got["a"][dead] == 7.5).all() and (got["r"][dead] == 9).all()


@pytest.mark.parametrize("name, form", BOTH)
def test_views(world, name, form):
    import torch
    sqt, O, ds = world["sqt"], world["O"], world["ds"]
    cams = [world["cam"], sqt.camera_from_text(ROTATED)]
    ds.set_lights(THREE)
    options(ds, **form)
    avg, rgb = ds.render_views(cams, 2, W, H, cast=True)
    torch.cuda.synchronize()
    avg, rgb = avg.cpu().numpy(), rgb.cpu().numpy()
    for i, cam in enumerate(cams):
        one = gpu_frame(world, 2, W, H, cam=cam)
        assert nan_eq(avg[i], one[0]).all() and np.array_equal(rgb[i], one[1]), f"view {i}"
    assert_frame((avg[0], rgb[0]), expected_frame(world, THREE, 2, W, H), "view 0")
    assert_frame((avg[1], rgb[1]), expected_frame(world, THREE, 2, W, H, ocam=O.camera_from_text(ROTATED), tag="rotated"), "view 1")


@pytest.mark.parametrize("name, form", BOTH)
def test_raycast_queries(world, name, form):
    import torch
    ds, cam = world["ds"], world["cam"]
    ds.set_lights(THREE)
    options(ds, **form)
    want = expected_frame(world, THREE, 1, W, H)
    frame = gpu_frame(world, 1, W, H)[0].reshape(-1, 3)
    assert nan_eq(frame, want[0].reshape(-1, 3)).all()
    o, d = ds.camera_rays(cam, W, H)
    o, d = o.reshape(-1, 3), d.reshape(-1, 3)
    rng = np.random.default_rng(5)
    lit_pixel = int(np.nonzero((want[2].reshape(-1, 3) != 0).any(-1))[0][7])
    for slots in (512 << 20, 64):                                      # 64: the wavefront form runs the 1000 rays in 16 chunks
        options(ds, **form, slots=slots)
        for idx in (np.array([lit_pixel]), np.arange(200, 265), rng.permutation(1000) % (W * H)):
            t = torch.from_numpy(idx).to(o.device)
            rad = ds.raycast(o[t], d[t])
            torch.cuda.synchronize()
            assert nan_eq(rad.cpu().numpy(), frame[idx]).all(), f"{len(idx)} rays, slots {slots}"
            assert (ds.last_plan()["trace_form"] != "per_pixel") == (form["cast_wavefront"] == 1)
    assert (frame[lit_pixel] != 0).any() and (frame[np.arange(200, 265)] != 0).any()


def test_odd_lights(world):
    """A light at a pixel's own hit point (dl = 0: power / 0, and a shadow ray without a direction), a NaN coordinate, a position
    near 1e30, and the powers 0, negative and +inf: inputs like any other.  (These lights are not held to the 10 lit / 10 shadowed
    rule of the fixture's lights: a NaN light lights nothing or everything by construction.)"""
    ds = world["ds"]
    key, rays = frame_rays(world, W, H)
    prim = world["R"].primary(key, rays)
    at = next(p for hit, p, _ in prim[300:] if hit)
    cases = {
        "at_a_hit_point": [(tuple(at), (2, 2, 2)), SIX[1]],
        "nan_coordinate": [SIX[1], ((float("nan"), 1, 1), (1, 2, 3))],
        "far": [((1e30, 0.5, -0.25), (1e30, 2e30, 3e30)), SIX[2]],
        "powers": [((0, 0, 0), (0, 0, 0)), ((1.5, -2, 0.5), (-1, -2, -0.5)), ((0, 3, -1), (float("inf"), 1, float("inf")))],
        "negative_first": [((0, 3, -1), (-1, -0.0, -3)), SIX[1]],
    }
    for what, lights in cases.items():
        want = expected_frame(world, lights, 2, W, H)
        ds.set_lights(lights)
        for name, form in BOTH:
            options(ds, **form)
            assert_frame(gpu_frame(world, 2, W, H), want, f"{what} {name}")


def test_order_and_lifetime(world):
    import torch
    ds, cam = world["ds"], world["cam"]
    # two lights alone commute (c_0 + c_1 = c_1 + c_0 in fp32): a third one between them makes the order of the fold visible
    ab, ba = [SIX[1], SIX[5], SIX[0]], [SIX[0], SIX[5], SIX[1]]
    want_ab, want_ba = expected_frame(world, ab, 1, W, H), expected_frame(world, ba, 1, W, H)
    assert not np.array_equal(want_ab[0].view(np.uint32), want_ba[0].view(np.uint32))      # the fold is ordered
    for name, form in BOTH:
        options(ds, **form)
        # the caller's array may be overwritten as soon as set_lights returns
        table = np.array([np.concatenate(as_light(li)) for li in ab], f32)
        ds.set_lights(table)
        table[:] = 77.0
        assert_frame(gpu_frame(world, 1, W, H), want_ab, f"ab {name}")
        # a frame enqueued before a later set_lights on the same stream keeps the earlier lights
        a1, r1 = ds.render_rows(cam, 1, W, H, cast=True)
        ds.set_lights(ba)
        a2, r2 = ds.render_rows(cam, 1, W, H, cast=True)
        torch.cuda.synchronize()
        assert_frame((a1.cpu().numpy(), r1.cpu().numpy()), want_ab, f"before the change, {name}")
        assert_frame((a2.cpu().numpy(), r2.cpu().numpy()), want_ba, f"ba {name}")


def test_refusals_change_nothing(world):
    import torch
    sqt, ds, cam = world["sqt"], world["ds"], world["cam"]
    L, N = sqt.lib(), sqt._native
    ds.set_lights(THREE)
    options(ds)
    before = ds.lights.copy()
    frame = gpu_frame(world, 1, W, H)
    many = (N.Light * 4097)()
    for lights, n in ((many, 4097), (many, -1), (None, 3), (many, 0)):
        assert L.sq_scene_set_lights(ds._h, lights, n, None) != 0
        assert len(L.sq_last_error()) > 0
        assert np.array_equal(ds.lights, before)
    with pytest.raises(sqt.SquiglyError):
        ds.set_lights(np.zeros((4097, 6), f32))
    assert L.sq_scene_set_lights(ds._h, many, 4096, None) == 0 and L.sq_scene_get_lights(ds._h, None, 0) == 4096
    ds.set_lights(THREE)
    got = gpu_frame(world, 1, W, H)
    assert nan_eq(got[0], frame[0]).all() and np.array_equal(got[1], frame[1])
    # a tree taller than the wavefront form takes: cast_wavefront 1 gets that form's refusal, cast_wavefront 0 renders it
    tall = sqt.DeviceScene(TP.height_with_chain(world["bih"], 200), 0)
    try:
        tall.set_lights(THREE)
        avg = torch.full((W, H, 3), 7.5, dtype=torch.float32, device="cuda:0")
        tall.set_option("cast_wavefront", 1)
        with pytest.raises(sqt.SquiglyError, match=r"BIH height 200 needs \d+ B of LDS per workgroup"):
            tall.render_rows(cam, 1, W, H, cast=True, out_avg=avg, want_rgb=False)
        torch.cuda.synchronize()
        assert (avg == 7.5).all() and tall.last_plan()["launched"] == 0
        assert np.array_equal(tall.lights, ds.lights)
        tall.set_option("cast_wavefront", 0)
        a, r = tall.render_rows(cam, 1, W, H, cast=True)
        torch.cuda.synchronize()
        assert nan_eq(a.cpu().numpy(), frame[0]).all() and np.array_equal(r.cpu().numpy(), frame[1])
    finally:
        tall.close()


def test_path_traced_frames_do_not_see_the_lights(world):
    import torch
    ds, cam = world["ds"], world["cam"]
    ds.set_lights(None)
    options(ds)
    a0, r0 = ds.render_rows(cam, 4, W, H)
    ds.set_lights(SIX)
    frames = []
    for wave in (0, 1):
        options(ds, cast_wavefront=wave)
        frames.append(ds.render_rows(cam, 4, W, H))
    torch.cuda.synchronize()
    for a, r in frames:
        assert torch.equal(a.view(torch.int32), a0.view(torch.int32)) and torch.equal(r, r0)
