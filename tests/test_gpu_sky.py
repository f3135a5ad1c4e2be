"""Caller-given sky on the GPU (sq_scene_set_sky, DeviceScene.set_sky): queries, folds, frames, masked and multi-view calls under a
sky equal tests/sky_restatement.py (pinned to depth_restatement and the oracle by tests/test_sky.py) bit for bit with NaN = NaN, at
every depth, in the per-lane form and around every trace form and primary form; a scene whose sky was reset runs what it ran before;
cast computations ignore the sky."""
import importlib
import os

import numpy as np
import pytest

import depth_restatement as DR
import sky_restatement as SR
from bitcmp import ibits, nan_eq
from conftest import DATA, GOLDEN, ROOT
from f32_folds import from_zero, tonemaps
from ray_oracle import raytrace
from render_options import FORM_IDS, PRIMARY_FORMS, SCENE_FORMS, primary_form_of, set_sky_options as set_options
from scenes import camera, open_case

pytestmark = pytest.mark.gpu
f32 = np.float32
DEPTHS = (1, 2, 3, 4, 5, 8)
INF_UP = ((np.inf, 0.5, 1.0), (0.75, 0.625, 0.5))
ZERO = ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))


def expected(s, depth, sky):
    key = (depth, sky)
    if key not in s.want:
        s.want[key] = from_zero(SR.radiances(s.paths, depth, sky))
    return s.want[key]


@pytest.fixture(scope="module")
def bright(sqt):
    s = open_case(sqt, DR.case("bright"), SR.case_paths)
    yield s
    s.ds.close()


@pytest.fixture(scope="module")
def shipped(sqt):
    s = open_case(sqt, DR.case("shipped"), SR.case_paths)
    yield s
    s.ds.close()


# ---- 1. queries ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts, form", SCENE_FORMS, ids=FORM_IDS)
def test_one_sample_under_a_sky_equals_the_restatement_at_every_depth_in_every_form(sqt, bright, opts, form):
    c, ds = bright.c, bright.ds
    try:
        for sky in (SR.GRADIENT, SR.CONSTANT):
            for slots in (512 << 20, 1024):                           # 1024: the 4000 rays run as four chunks
                for depth in DEPTHS:
                    set_options(ds, sky=sky, depth=depth, **{**opts, "slots": slots})   # deep 0: D = 3 too takes the generic form
                    assert ds.sky == sky and ds.depth == depth
                    ds.reset_timing()
                    ds.enable_timing(True)
                    got = raytrace(ds, c.o, c.d, c.s)[0]
                    launches, kernel = ds.kernel_timing()[1:3]
                    ds.enable_timing(False)
                    want = expected(bright, depth, sky)
                    ok = nan_eq(got, want).all(-1)
                    assert ok.all(), (form, sky, slots, depth, int((~ok).sum()), np.nonzero(~ok)[0][:8])
                    plan = ds.last_plan()
                    assert plan["trace_form"] == form and plan["launched"] == 1 and plan["primary_form"] == primary_form_of(form, opts), plan
                    assert plan["n_emitters"] == -1                  # no emitter pre-test under a sky
                    if form != "per_pixel" and slots != 1024 and depth >= 2:   # the generic form: one trace launch per bounce level, D = 3 included
                        assert launches == depth - 1, (depth, launches)
                    elif form == "per_pixel":
                        assert "deep_sky" in kernel, kernel
        assert (ibits(expected(bright, 3, SR.GRADIENT)) != ibits(expected(bright, 3, None))).any(-1).mean() > 0.25
    finally:
        set_options(ds)


def test_one_sample_on_the_shipped_materials_in_the_default_form(sqt, shipped):
    c, ds = shipped.c, shipped.ds
    try:
        for depth in DEPTHS:
            set_options(ds, sky=SR.GRADIENT, depth=depth)
            got = raytrace(ds, c.o, c.d, c.s)[0]
            ok = nan_eq(got, expected(shipped, depth, SR.GRADIENT)).all(-1)
            assert ok.all(), (depth, int((~ok).sum()), np.nonzero(~ok)[0][:8])
    finally:
        set_options(ds)


# ---- 2. a fold -------------------------------------------------------------------------------------------------------
def test_a_fold_of_eight_samples_at_depth_5_under_a_sky_in_ranges_and_batches(sqt, O, bright):
    import torch
    c = bright.c
    idx = np.arange(0, len(c.o), 4)                                   # 1000 rays, every family
    o, d, sd = c.o[idx], c.d[idx], c.s[idx]
    sky = SR.GRADIENT
    rs = [SR.radiances([bright.paths[i] for i in idx], 5, sky)] + [SR.radiances(SR.paths(c.ob, c.flat, o, d, sd, k=k), 5, sky) for k in range(1, 8)]
    want_sum = np.zeros_like(rs[0])
    with np.errstate(all="ignore"):
        for r in rs:
            want_sum = (want_sum + r).astype(f32)
        want_avg = ((f32(1) / f32(8)) * want_sum).astype(f32)
    want_rgb = tonemaps(O, want_avg)
    miss0 = np.array([isinstance(bright.paths[i][0], SR.Miss) for i in idx])
    assert miss0.sum() >= 50
    eight = np.zeros(3, f32)
    for i in np.nonzero(miss0)[0][:5]:                                # a level-0 miss folds eight additions of sky(d_0), not 8 * sky
        eight[:] = 0
        for _ in range(8):
            eight = (eight + SR.sky_of(sky, d[i])).astype(f32)
        assert np.array_equal(ibits(eight), ibits(want_sum[i]))
    assert any(not np.array_equal(ibits(want_sum[i]), ibits((f32(8) * SR.sky_of(sky, d[i])).astype(f32))) for i in np.nonzero(miss0)[0])
    for opts in ({}, {"variant": 1}, {"resident": 0, "trace_blocks_per_cu": 1}):
        ds = sqt.DeviceScene(c.bih, 0)                                # a workspace that never held more: 3 samples per batch
        try:
            set_options(ds, sky=sky, depth=5, slots=3 * len(o), **opts)
            whole = raytrace(ds, o, d, sd, samples=8, want_rgb=True)
            for g, e, name in zip(whole, (want_sum, want_avg, want_rgb), ("sum", "avg", "rgb")):
                assert nan_eq(g, e).all() if g.dtype == f32 else np.array_equal(g, e), (opts, name)
            sums = None
            for k0, k1 in ((0, 3), (3, 8)):
                r = ds.raytrace(o, d, seeds=sd, samples=8, k_range=(k0, k1), sums=sums, want_rgb=True)
                sums = r.sum
            torch.cuda.synchronize()
            for g, e in zip(r, whole):
                assert np.array_equal(g.cpu().numpy().view(np.uint8), e.view(np.uint8)), opts
        finally:
            ds.close()


# ---- 3. frames -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cam_name", ("camera", "rotated"))
@pytest.mark.parametrize("w, h", ((16, 24), (40, 72)))
def test_a_frame_under_a_sky_equals_the_restatements_frame_and_the_query_of_its_rays(sqt, O, bright, w, h, cam_name):
    import torch
    ds, spp, sky = bright.ds, 3, SR.GRADIENT
    cam = camera(sqt, cam_name)
    fp = SR.frame_case("bright", cam_name, w, h, spp)
    miss = np.array([isinstance(t[0], SR.Miss) for t in fp[0]]).reshape(w, h)
    assert miss.sum() >= 20 and (~miss).sum() >= 20
    try:
        for depth in (1, 3, 5):
            _, _, avg_all = SR.fold_frame(fp, depth, sky)
            avg_all = avg_all.reshape(w, h, 3)
            assert (avg_all[miss] != 0).all()                         # no pixel is black under this sky
            for shard in ((None, 0, 1), (2, 1, 3)):
                want = avg_all[DR.shard_rows(w, shard)]
                want_rgb = tonemaps(O, want)
                for opts, primary in PRIMARY_FORMS:
                    set_options(ds, sky=sky, depth=depth, **opts)
                    avg, rgb = ds.render_rows(cam, spp, w, h, shard=shard)
                    torch.cuda.synchronize()
                    what = (depth, shard, opts)
                    assert ds.last_plan()["primary_form"] == primary and ds.last_plan()["launched"] == 1, what
                    assert np.array_equal(ibits(avg.cpu().numpy()), ibits(want)), what
                    assert np.array_equal(rgb.cpu().numpy(), want_rgb), what
                set_options(ds, sky=sky, depth=depth)
                q = ds.raytrace(*ds.camera_rays(cam, w, h, shard=shard), seeds=sqt.frame_seeds(spp, w, h, shard=shard, device="cuda:0"),
                                samples=spp, want_rgb=True)
                torch.cuda.synchronize()
                assert np.array_equal(ibits(q.avg.cpu().numpy()), ibits(want)) and np.array_equal(q.rgb.cpu().numpy(), want_rgb), (depth, shard)
    finally:
        set_options(ds)


def test_a_progressive_frame_in_three_ranges_equals_the_whole_frame_and_carries_the_sky(sqt, bright):
    import torch
    device = importlib.import_module("squigly-trace_amd.device")
    ds, w, h, spp, sky = bright.ds, 16, 24, 3, SR.GRADIENT
    cam = camera(sqt, "camera")
    _, _, want = SR.fold_frame(SR.frame_case("bright", "camera", w, h, spp), 3, sky)
    try:
        for opts in ({}, {"primary_pooled": 1}, {"variant": 1}):
            set_options(ds, sky=sky, **opts)
            p = device.Progressive(ds, cam, spp, w, h)
            assert p.sky == sky
            for _ in range(3):
                avg, _ = p.step(1)
            torch.cuda.synchronize()
            assert p.finished and np.array_equal(ibits(avg.cpu().numpy()), ibits(want.reshape(w, h, 3))), opts
        set_options(ds, sky=sky)
        p = device.Progressive(ds, cam, spp, w, h)
        p.step(1)
        sums, done = p.sums.clone(), p.done
        for other in (None, SR.CONSTANT):
            set_options(ds, sky=other)
            with pytest.raises(sqt.SquiglyError, match="sky"):
                p.step(1)
            with pytest.raises(sqt.SquiglyError, match="sky"):
                device.Progressive(ds, cam, spp, w, h, sums=sums, done=done, sky=sky)
            with pytest.raises(sqt.SquiglyError, match="sky"):
                device.Adaptive(ds, cam, spp, w, h, 0.1, sky=sky)
        with pytest.raises(sqt.SquiglyError, match="sky"):
            device.Progressive(ds, cam, spp, w, h, sums=sums, done=done, sky=None)   # a checkpoint without a sky, a scene with one
        set_options(ds, sky=sky)
        r = device.Progressive(ds, cam, spp, w, h, sums=sums, done=done, sky=sky)
        avg, _ = r.step(2)
        a = device.Adaptive(ds, cam, spp, w, h, 0.0, first=spp)
        assert a.sky == sky
        avg_a, _ = a.step()
        torch.cuda.synchronize()
        for got in (avg, avg_a):
            assert np.array_equal(ibits(got.cpu().numpy()), ibits(want.reshape(w, h, 3)))
        pc = device.Progressive(ds, cam, spp, w, h, cast=True)        # a cast frame neither records the sky nor minds a change of it
        pc.step(1)
        ds.set_sky(None)
        pc.step(2)
        assert pc.sky is None and pc.finished
    finally:
        set_options(ds)


# ---- 4. masked calls and views ---------------------------------------------------------------------------------------
def test_a_masked_call_at_depth_4_under_a_sky_holds_the_moments_and_leaves_dead_pixels_alone(sqt, O, bright):
    import torch
    ds, w, h, spp, depth, sky = bright.ds, 16, 24, 3, 4, SR.GRADIENT
    cam = camera(sqt, "camera")
    fp = SR.frame_case("bright", "camera", w, h, spp)
    want_sum, want_sum2, want_avg = (a.reshape(w, h, 3) for a in SR.fold_frame(fp, depth, sky))
    want_rgb = tonemaps(O, want_avg)
    miss = np.array([isinstance(t[0], SR.Miss) for t in fp[0]]).reshape(w, h)
    live = (np.add.outer(np.arange(w), np.arange(h)) % 2 == 0)
    assert (live & miss).sum() >= 20 and (live & ~miss).sum() >= 20 and (~live & miss).sum() >= 20
    assert (want_sum2[live & miss] != 0).all()
    try:
        for opts in ({}, {"variant": 1}, {"resident": 0, "trace_blocks_per_cu": 1}, {"primary_resident": 0}, {"primary_pooled": 1}):
            set_options(ds, sky=sky, depth=depth, **opts)
            mask = torch.from_numpy(live.astype(np.uint8)).cuda()
            sums = torch.full((w, h, 3), 5.5, dtype=torch.float32, device="cuda:0")
            sums2 = torch.full((w, h, 3), -6.5, dtype=torch.float32, device="cuda:0")
            counts = torch.full((w, h), 77, dtype=torch.int32, device="cuda:0")
            avg = torch.full((w, h, 3), 8.25, dtype=torch.float32, device="cuda:0")
            rgb = torch.full((w, h, 3), 99, dtype=torch.uint8, device="cuda:0")
            ds.render_rows_masked(cam, spp, w, h, 0, spp, sums, mask=mask, sums2=sums2, counts=counts, out_avg=avg, out_rgb=rgb)
            torch.cuda.synchronize()
            s, q, n, a, r = (t.cpu().numpy() for t in (sums, sums2, counts, avg, rgb))
            assert np.array_equal(ibits(s[live]), ibits(want_sum[live])), opts
            assert np.array_equal(ibits(q[live]), ibits(want_sum2[live])), opts
            assert (n[live] == spp).all()
            assert np.array_equal(ibits(a[live]), ibits(want_avg[live])) and np.array_equal(r[live], want_rgb[live]), opts
            assert (s[~live] == 5.5).all() and (q[~live] == -6.5).all() and (n[~live] == 77).all(), opts
            assert (a[~live] == 8.25).all() and (r[~live] == 99).all(), opts
    finally:
        set_options(ds)


def test_two_cameras_in_one_views_call_under_a_sky_equal_their_single_view_frames(sqt, bright):
    import torch
    ds, w, h, spp, sky = bright.ds, 16, 24, 3, SR.GRADIENT
    cams = [camera(sqt, "camera"), camera(sqt, "rotated")]
    try:
        for opts in ({}, {"variant": 1}, {"primary_resident": 0}, {"primary_pooled": 1}):
            set_options(ds, sky=sky, depth=4, **opts)
            avg, rgb = ds.render_views(cams, spp, w, h)
            singles = [ds.render_rows(c, spp, w, h) for c in cams]
            torch.cuda.synchronize()
            for i, (a, r) in enumerate(singles):
                assert np.array_equal(ibits(avg[i].cpu().numpy()), ibits(a.cpu().numpy())) and torch.equal(rgb[i], r), (opts, i)
            _, _, want = SR.fold_frame(SR.frame_case("bright", "rotated", w, h, spp), 4, sky)
            assert np.array_equal(ibits(avg[1].cpu().numpy()), ibits(want.reshape(w, h, 3))), opts
    finally:
        set_options(ds)


# ---- 5. odd skies ----------------------------------------------------------------------------------------------------
ODD_SKIES = (("inf up", INF_UP), ("nan", ((0.25, np.nan, 1.0), (0.75, 0.625, 0.5))), ("negative", ((0.25, 0.5, 1.0), (-0.75, 0.625, -0.5))),
             ("zero", ZERO))


def test_infinite_nan_negative_and_zero_skies(sqt, bright):
    c, ds = bright.c, bright.ds
    absorbing = np.array([SR.absorbing_above_miss(t, 3) for t in bright.paths])
    zero_d = (c.d == 0).all(-1)
    assert c.families[3] == "degenerate" and zero_d[3 * DR.N_RAYS:].sum() >= 5 and absorbing.sum() >= 10
    try:
        for name, sky in ODD_SKIES:
            for depth in (3, 5):
                want = expected(bright, depth, sky)
                if name == "inf up" and depth == 3:                   # 0 * inf below an absorbing hit is the reference's NaN
                    assert np.isnan(want[absorbing][:, 0]).sum() >= 10 and np.isinf(want[:, 0]).any()
                if name == "zero":                                    # a sky of all +0 is a sky: NaN on the rays with d = 0, black's bits elsewhere
                    none = expected(bright, depth, None)
                    assert np.isnan(want[zero_d]).all() and not np.isnan(none[zero_d]).any()
                for opts in ({}, {"variant": 1}, {"resident": 0, "trace_blocks_per_cu": 1}, {"primary_pooled": 1}):
                    set_options(ds, sky=sky, depth=depth, **opts)
                    got = raytrace(ds, c.o, c.d, c.s)[0]
                    ok = nan_eq(got, want).all(-1)
                    assert ok.all(), (name, depth, opts, int((~ok).sum()), np.nonzero(~ok)[0][:8])
    finally:
        set_options(ds)


def test_odd_skies_over_odd_materials(sqt):
    c = DR.case("odd")
    trails = SR.case_paths(c)
    ds = sqt.DeviceScene(c.bih, 0)
    try:
        for name, sky in ODD_SKIES:
            want = from_zero(SR.radiances(trails, 4, sky))
            assert np.isnan(want).any()
            for opts in ({}, {"variant": 1}, {"resident": 0, "trace_blocks_per_cu": 1}):
                set_options(ds, sky=sky, depth=4, **opts)
                got = raytrace(ds, c.o, c.d, c.s)[0]
                ok = nan_eq(got, want).all(-1)
                assert ok.all(), (name, opts, int((~ok).sum()), np.nonzero(~ok)[0][:8])
    finally:
        ds.close()


# ---- 6. reset, and cast ----------------------------------------------------------------------------------------------
def test_after_a_reset_the_goldens_come_out_by_the_kernels_of_before_and_cast_ignores_the_sky(sqt, shipped):
    import torch
    c = shipped.c
    cam = camera(sqt, "camera")
    golden = np.load(os.path.join(GOLDEN, "scene_64x64_4spp_avg.npy"))
    golden8 = np.load(os.path.join(GOLDEN, "scene_64x64_4spp_rgb8.npy"))
    ds = sqt.DeviceScene(c.bih, 0)
    try:
        set_options(ds)
        assert ds.sky is None
        first, _ = ds.render_rows(cam, 4, 64, 64)
        cast0, cast0_8 = ds.render_rows(cam, 2, 64, 64, cast=True)
        rc0 = ds.raycast(c.o, c.d)
        torch.cuda.synchronize()
        cover = ds.rng_table()[0]
        assert cover > 0
        ds.set_sky(*SR.GRADIENT)
        assert ds.sky == SR.GRADIENT
        under, _ = ds.render_rows(cam, 4, 64, 64)
        cast1, cast1_8 = ds.render_rows(cam, 2, 64, 64, cast=True)
        rc1 = ds.raycast(c.o, c.d)
        torch.cuda.synchronize()
        assert not np.array_equal(ibits(under.cpu().numpy()), ibits(golden.reshape(64, 64, 3)))
        assert ds.rng_table()[0] == cover                              # a sky frame reads the table and never grows it
        assert torch.equal(cast1, cast0) and torch.equal(cast1_8, cast0_8) and cast0.any()
        assert np.array_equal(ibits(rc1.cpu().numpy()), ibits(rc0.cpu().numpy()))
        ds.set_sky(ZERO[0])                                            # all +0 is a sky still: the generic form, without the emitter pre-test
        assert ds.sky == ZERO
        ds.reset_timing()
        ds.enable_timing(True)
        ds.render_rows(cam, 4, 64, 64)
        torch.cuda.synchronize()
        assert ds.kernel_timing()[1] == 2 and ds.last_plan()["n_emitters"] == -1
        ds.set_sky(None)
        assert ds.sky is None
        ds.reset_timing()
        again, again8 = ds.render_rows(cam, 4, 64, 64)
        torch.cuda.synchronize()
        assert ds.kernel_timing()[1] == 2                               # the three-level pipeline's two trace launches
        assert ds.last_plan()["n_emitters"] >= 0 and ds.last_plan()["level1_cull"] == 1
        ds.enable_timing(False)
        assert ds.rng_table()[0] == cover
        for a in (first, again):
            assert np.array_equal(ibits(a.cpu().numpy()), ibits(golden.reshape(64, 64, 3)))
        assert np.array_equal(again8.cpu().numpy(), golden8.reshape(64, 64, 3))
    finally:
        ds.close()


def test_null_sky_through_the_c_call_and_the_getter(sqt, bright):
    import ctypes
    L, ds = sqt.lib(), bright.ds
    out = (ctypes.c_float * 6)(9, 9, 9, 9, 9, 9)
    try:
        set_options(ds)
        assert L.sq_scene_get_sky(ds._h, out) == 0 and list(out) == [9] * 6
        ds.set_sky((1, 2, 3), (4, 5, float("inf")))
        assert L.sq_scene_get_sky(ds._h, None) == 1
        assert L.sq_scene_get_sky(ds._h, out) == 1 and list(out) == [1, 2, 3, 4, 5, float("inf")]
        assert L.sq_scene_set_sky(None, out) != 0 and ds.sky == ((1.0, 2.0, 3.0), (4.0, 5.0, float("inf")))
    finally:
        set_options(ds)


# ---- 7. streams ------------------------------------------------------------------------------------------------------
def test_a_sky_frame_and_a_sky_query_on_a_gated_side_stream(sqt, O, product_scene, oracle_scene):
    import torch
    import stream_harness as S
    env = S.Env(sqt, torch, O, product_scene[0], oracle_scene[0])
    try:
        for form in ("default", "variant1", "resident0"):
            env.set_options(env.ds, **S.FORMS[form])
            env.ds.set_sky(*SR.GRADIENT)
            frames = S.drive(env, S.job_frames(env, env.ds), env.side, f"sky frames-{form}")
            rays = S.drive(env, S.job_raytrace(env, env.ds), env.side, f"sky raytrace-{form}")
            assert frames["avg0"].any() and rays["rsum"].any()
            env.ds.set_sky(None)
            torch.cuda.synchronize()
            three = S.plain(env, S.job_frames(env, env.ds))[0]
            assert np.array_equal(S.bits(three["avg0"]), S.bits(S.golden("scene_64x64_4spp_avg.npy").reshape(three["avg0"].shape)))
            assert not np.array_equal(S.bits(three["avg0"]), S.bits(frames["avg0"]))       # the sky frame was under the sky
    finally:
        env.ds.set_sky(None)
        env.set_options(env.ds)
        env.close()


# ---- 8. random scenes ------------------------------------------------------------------------------------------------
BLOCK = 25
BLOCKS = [range(first, first + BLOCK) for first in range(1000, 1100, BLOCK)]


def run_sky_case(sqt, seed):
    """fuzz_features.case(seed) under its drawn depth and sky_restatement.fuzz_sky(seed): the frame in variant 2 and 1, the ray batch in
    the drawn form and in variant 1, a masked call.  Returns the mismatch messages; a refusal is one."""
    import torch
    import fuzz_features as FF
    c = FF.case(seed)
    sky, D = SR.fuzz_sky(seed), c.depth
    bad = []
    cam = sqt.camera_from_text(c.camt)
    w, h, spp, shard, rows = c.w, c.h, c.spp, c.shard, len(c.rows)
    shape = (rows, h, 3)
    want_s, want_q, want = (a.reshape(shape) for a in SR.fold_frame(SR.fuzz_frame_paths(c), D, sky))
    want8 = FF.tonemaps(want)
    ro, rd, rs = FF.radiance_rays(c)
    want_rays = FF.from_zero(SR.radiances(SR.fuzz_ray_paths(c), D, sky))
    ds = sqt.DeviceScene(FF.product_bih(c), 0)
    try:
        for k, val in c.knobs.items():
            ds.set_option(k, val)
        ds.set_option("slots", c.slots)
        ds.set_option("deep", c.deep)
        ds.set_depth(D)
        ds.set_sky(*sky)
        for variant in (2, 1):
            ds.set_option("variant", variant)
            avg, rgb = ds.render_rows(cam, spp, w, h, shard=shard)
            torch.cuda.synchronize()
            if not FF.same(avg.cpu().numpy(), want):
                bad.append(f"frame, depth {D}, variant {variant}: avg differs in {int((FF.canon(avg.cpu().numpy()) != FF.canon(want)).any(-1).sum())}/{rows * h} pixels")
            elif not np.array_equal(rgb.cpu().numpy(), want8):
                bad.append(f"frame, depth {D}, variant {variant}: rgb8 differs")
            if ds.last_plan()["launched"] != 1:
                bad.append(f"frame, variant {variant}: plan says launched = {ds.last_plan()['launched']}")
            got = ds.raytrace(ro, rd, seeds=rs).sum
            torch.cuda.synchronize()
            if not FF.same(got.cpu().numpy(), want_rays):
                bad.append(f"raytrace of {len(ro)} rays, depth {D}, variant {variant}: {int((FF.canon(got.cpu().numpy()) != FF.canon(want_rays)).any(-1).sum())} rays differ")
        ds.set_option("variant", 2)
        live = c.live
        dev = "cuda:0"
        mask = torch.from_numpy(live.astype(np.uint8)).to(dev)
        sums = torch.full(shape, 5.5, dtype=torch.float32, device=dev)
        sums2 = torch.full(shape, -6.5, dtype=torch.float32, device=dev)
        counts = torch.full((rows, h), 77, dtype=torch.int32, device=dev)
        avg = torch.full(shape, 8.25, dtype=torch.float32, device=dev)
        rgb = torch.full(shape, 99, dtype=torch.uint8, device=dev)
        ds.render_rows_masked(cam, spp, w, h, 0, spp, sums, mask=mask, sums2=sums2, counts=counts, shard=shard, out_avg=avg, out_rgb=rgb)
        torch.cuda.synchronize()
        s, q2, n, a, r = (t.cpu().numpy() for t in (sums, sums2, counts, avg, rgb))
        if not (FF.same(s[live], want_s[live]) and FF.same(q2[live], want_q[live]) and (n[live] == spp).all()
                and FF.same(a[live], want[live]) and np.array_equal(r[live], want8[live])):
            bad.append(f"masked call, depth {D}: a live pixel differs from the restatement's sum, sum2, count, avg or rgb")
        dead = ~live
        if not ((s[dead] == 5.5).all() and (q2[dead] == -6.5).all() and (n[dead] == 77).all() and (a[dead] == 8.25).all() and (r[dead] == 99).all()):
            bad.append(f"masked call, depth {D}: a dead pixel lost a sentinel")
    except sqt.SquiglyError as e:
        if " failed: " in str(e):                                       # a HIP error is no refusal: nothing more runs on this device
            FF.DEVICE_ERROR.append(f"seed {seed}: {e}")
            raise
        bad.append(f"refused: {e}")
    finally:
        ds.close()
    return bad


@pytest.mark.parametrize("seeds", BLOCKS, ids=[f"{b[0]}-{b[-1]}" for b in BLOCKS])
def test_a_block_of_random_scenes_under_their_skies(sqt, seeds):
    import fuzz_features as FF
    assert not FF.DEVICE_ERROR, FF.DEVICE_ERROR
    failures = [(seed, msg) for seed in seeds for msg in run_sky_case(sqt, seed)]
    assert not failures, failures


# ---- 9. the CLIs -----------------------------------------------------------------------------------------------------
def test_both_clis_render_a_sky_frame_equal_to_the_device_scenes(sqt, tmp_path, product_scene):
    import subprocess
    import torch
    from PIL import Image
    bih, cam, _ = product_scene
    ds = sqt.DeviceScene(bih, 0)
    try:
        plain = ds.render_rows(cam, 4, 48, 40, want_avg=False)[1].cpu().numpy()
        ds.set_sky(*SR.GRADIENT)
        want = ds.render_rows(cam, 4, 48, 40, want_avg=False)[1].cpu().numpy()
        ds.set_depth(2)
        want2 = ds.render_rows(cam, 4, 48, 40, want_avg=False)[1].cpu().numpy()
        torch.cuda.synchronize()
    finally:
        ds.close()
    assert not np.array_equal(want, plain) and not np.array_equal(want2, want)
    exe = os.path.join(ROOT, "squigly-trace_amd", "bin", "squigly-trace")
    out = str(tmp_path / "sky.png")
    cli = importlib.import_module("squigly-trace_amd.cli")
    cwd = os.getcwd()
    text = "0.25,0.5,1,0.75,0.625,0.5"
    for extra, exp in (([], want), (["--depth", "2"], want2)):
        r = subprocess.run([exe, "-s", "4", "-d", "48,40", "-p", out, "--sky", text] + extra, cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert np.array_equal(np.array(Image.open(out).convert("RGB")), exp), ("c++", extra)
        os.remove(out)
        os.chdir(ROOT)
        try:
            assert cli.main(["-s", "4", "-d", "48,40", "-p", out, f"--sky={text}"] + extra) == 0
        finally:
            os.chdir(cwd)
        assert np.array_equal(np.array(Image.open(out).convert("RGB")), exp), ("python", extra)
        os.remove(out)
