"""Radiance queries on a resident scene (sq_raytrace_rays_device, sq_raycast_rays_device, DeviceScene.raytrace / raycast): every ray's
fold of sample radiances is bit for bit the oracle's Lib.raytrace (src/Lib.hs:127-137) with the caller's ray and seed, in every
trace form and option; a frame is the query of its camera rays with its seeds; Lib.raycast (src/Lib.hs:141-151) likewise.

The oracle has no entry point for a caller-given ray.  Its raytrace is reached through sample_radiance with a camera that is not a
rotation: pos = o, rot = [dx, dy, dz, 0, 0, 0, 0, 0, 0] makes rotVert return d for every pixel, and with w = h = 1, y = 0,
samples = N, x = seed div N, k = seed mod N the generator is mkTFGen seed.  A -0.0 direction component would come out as +0.0
(-0 + 0), so the families below hold no negative-zero direction components."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import render_options as RO
import tree_padding as TP
from bitcmp import ibits, nan_eq
from conftest import DATA, GOLDEN
from f32_folds import fold_list as fold
from ray_oracle import N_FAMILY, RADIANCE_FAMILIES as FAMILIES, cast_from_queries, make_radiance_families as make_families, oracle_raycast, oracle_raytrace, raytrace
from render_options import FORM_IDS, SCENE_FORMS, primary_form_of
from scenes import BRIGHT_SQ, ROTATED

pytestmark = pytest.mark.gpu
f32 = np.float32
set_options = functools.partial(RO.set_options, table=RO.RADIANCE)


def nonzero_share(r):
    with np.errstate(all="ignore"):
        return float(((r != 0) & ~np.isnan(r)).any(-1).mean())


class Case:
    """One scene: product BIH, oracle BIH, device scene, families, seeds and the oracle's one-sample radiances."""


def build_case(sqt, O, sq_text, seed):
    obj = open(os.path.join(DATA, "scene.obj"), "rb").read()
    c = Case()
    c.bih = sqt.BIH(sqt.Mesh.from_text(obj, sq_text))
    c.otris = O.tris_from_text(obj, sq_text)
    c.ob = O.BIH(c.otris)
    c.fam, c.seeds = make_families(c.bih, c.ob.flatten(), seed)
    c.exp = {k: oracle_raytrace(O, c.ob, *c.fam[k], c.seeds[k]) for k in FAMILIES}
    c.ds = sqt.DeviceScene(c.bih, 0)
    return c


@pytest.fixture(scope="module")
def shipped(sqt, O):
    c = build_case(sqt, O, open(os.path.join(DATA, "scene.sq"), "rb").read(), 11)
    # the inputs, judged by the oracle alone: a test on these rays cannot pass on black
    share = {k: nonzero_share(c.exp[k]) for k in FAMILIES}
    print("shipped scene, share of rays with non-zero one-sample radiance:", share)
    assert share["free"] >= 0.01 and share["surface"] >= 0.01 and share["to_light"] >= 0.25, share
    yield c
    c.ds.close()


@pytest.fixture(scope="module")
def bright(sqt, O):
    c = build_case(sqt, O, BRIGHT_SQ, 12)
    r = c.exp["free"]
    share = nonzero_share(r)
    distinct = len(np.unique(ibits(r[(r != 0).any(-1)]), axis=0))
    moved = oracle_raytrace(O, c.ob, *c.fam["free"], c.seeds["free"], k=1)
    hitting = (r != 0).any(-1) | (moved != 0).any(-1)
    sensitive = float((ibits(r) != ibits(moved)).any(-1)[hitting].mean())
    print(f"bright variant, free rays: {share:.3f} non-zero, {distinct} distinct radiances, {sensitive:.3f} of the hitting rays change with seed + 1")
    assert share >= 0.30 and distinct >= 50 and sensitive >= 0.30, (share, distinct, sensitive)
    yield c
    c.ds.close()


def all_rays(c):
    return (np.concatenate([c.fam[k][0] for k in FAMILIES]), np.concatenate([c.fam[k][1] for k in FAMILIES]),
            np.concatenate([c.seeds[k] for k in FAMILIES]))


def check_one_sample(c, what):
    o, d, s = all_rays(c)
    got = raytrace(c.ds, o, d, s)[0]
    for i, k in enumerate(FAMILIES):
        sl = slice(i * N_FAMILY, (i + 1) * N_FAMILY)
        with np.errstate(all="ignore"):
            want = (f32(0) + c.exp[k]).astype(f32)
        ok = nan_eq(got[sl], want).all(-1)
        assert ok.all(), (what, k, int((~ok).sum()), np.nonzero(~ok)[0][:8])


# ---- 1. one sample against the oracle --------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ("shipped", "bright"))
@pytest.mark.parametrize("opts, form", SCENE_FORMS, ids=FORM_IDS)
def test_one_sample_equals_the_oracles_raytrace_in_every_form(request, which, opts, form):
    c = request.getfixturevalue(which)
    try:
        for cull in (0, 1):
            set_options(c.ds, cull=cull, **opts)
            check_one_sample(c, (which, form, opts, cull))
            plan = c.ds.last_plan()
            assert plan["trace_form"] == form and plan["launched"] == 1 and plan["primary_form"] == primary_form_of(form, opts), plan
            assert (plan["n_emitters"] >= 0) == (which == "shipped"), plan      # the emitter list is off on the bright variant
    finally:
        set_options(c.ds)


# ---- 2. a fold against the oracle ------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ("to_light", "free"))
def test_a_fold_of_eight_samples_equals_the_oracles_fold_average_and_tonemap(O, bright, family):
    c = bright
    set_options(c.ds)
    n = 2000
    o, d, s = c.fam[family][0][:n], c.fam[family][1][:n], c.seeds[family][:n]
    rs = [c.exp[family][:n]] + [oracle_raytrace(O, c.ob, o, d, s, k=k) for k in range(1, 8)]
    want_sum = fold(rs)
    with np.errstate(all="ignore"):
        want_avg = ((f32(1) / f32(8)) * want_sum).astype(f32)
    want_rgb = np.array([O.tonemap(a) for a in want_avg], np.uint8)
    assert (want_sum != 0).any(-1).mean() > 0.3
    got_sum, got_avg, got_rgb = raytrace(c.ds, o, d, s, samples=8, want_rgb=True)
    assert nan_eq(got_sum, want_sum).all(), int((~nan_eq(got_sum, want_sum)).any(-1).sum())
    assert nan_eq(got_avg, want_avg).all()
    assert np.array_equal(got_rgb, want_rgb), int((got_rgb != want_rgb).any(-1).sum())


# ---- 3. a frame is a query -------------------------------------------------------------------------------------------
def frame_option_sets(n_rays):
    return ([o for o, _ in SCENE_FORMS] +
            [{"overlap": 1}, {"overlap": 2}, {"primary_pooled": 1}, {"primary_resident": 0}, {"pixel_major": 0}, {"pixel_major": 1},
             {"slots": n_rays}, {"overlap": 2, "slots": 2 * n_rays}, {"overlap": 1, "slots": 2 * n_rays, "primary_pooled": 1}])


@pytest.mark.parametrize("shard", ((None, 0, 1), (2, 1, 3)), ids=("whole", "shard"))
@pytest.mark.parametrize("w, h, spp", ((64, 64, 4), (40, 72, 3)))
@pytest.mark.parametrize("camera", ("camera", "rotated"))
def test_a_frame_is_the_query_of_its_camera_rays_with_its_seeds(sqt, shipped, camera, w, h, spp, shard):
    import torch
    ds = shipped.ds
    cam = sqt.camera_from_text(open(os.path.join(DATA, "camera"), "rb").read() if camera == "camera" else ROTATED)
    try:
        set_options(ds)
        avg, rgb = ds.render_rows(cam, spp, w, h, shard=shard)
        sums = torch.empty_like(avg)
        ds.render_rows_range(cam, spp, w, h, 0, spp, sums, shard=shard)
        o, d = ds.camera_rays(cam, w, h, shard=shard)
        seeds = sqt.frame_seeds(spp, w, h, shard=shard, device="cuda:0")
        torch.cuda.synchronize()
        want = tuple(t.cpu().numpy() for t in (sums, avg, rgb))
        assert want[1].any()
        if camera == "camera" and shard == (None, 0, 1):
            golden = np.load(os.path.join(GOLDEN, f"scene_{w}x{h}_{spp}spp_avg.npy"))
            assert np.array_equal(ibits(want[1]), ibits(golden.reshape(want[1].shape)))
        n_rays = o.shape[0] * o.shape[1]
        for opts in frame_option_sets(n_rays):
            # the workspace only grows, and a frame batches by what the workspace holds: `slots` forces several sample batches on a
            # scene whose workspace has never been larger
            q = sqt.DeviceScene(shipped.bih, 0) if "slots" in opts else ds
            try:
                set_options(q, **opts)
                q.reset_timing()
                q.enable_timing(True)
                got = raytrace(q, o, d, seeds, samples=spp, want_rgb=True)
                launches = q.kernel_timing()[1]
                q.enable_timing(False)
                q.reset_timing()
                assert got[0].shape == want[0].shape and got[2].dtype == np.uint8
                for g, e, name in zip(got, want, ("sum", "avg", "rgb")):
                    assert np.array_equal(ibits(g) if g.dtype == f32 else g, ibits(e) if e.dtype == f32 else e), (opts, name)
                assert q.last_plan()["launched"] == 1
                if opts == {"slots": n_rays}:                     # one sample per batch: spp batches of two trace launches
                    assert launches == 2 * spp, launches
                elif "slots" in opts:
                    assert launches >= 2 * spp, (opts, launches)
            finally:
                if q is not ds:
                    q.close()
    finally:
        set_options(ds)


# ---- 4. ranges -------------------------------------------------------------------------------------------------------
def test_consecutive_ranges_equal_one_call_and_missing_rays_stay_zero(bright):
    import torch
    c = bright
    set_options(c.ds)
    o, d, s = all_rays(c)
    whole = raytrace(c.ds, o, d, s, samples=8, want_rgb=True)
    sums = None
    for k0, k1 in ((0, 3), (3, 4), (4, 8)):
        r = c.ds.raytrace(o, d, seeds=s, samples=8, k_range=(k0, k1), sums=sums, want_rgb=True)
        assert sums is None or r.sum is sums
        sums = r.sum
    torch.cuda.synchronize()
    for g, e in zip(r, whole):
        g = g.cpu().numpy()
        assert nan_eq(g, e).all() if g.dtype == f32 else np.array_equal(g, e)
    miss = (c.ds.intersect(o, d).tri < 0).cpu().numpy()
    assert miss.sum() > 1000
    om, dm, sm = o[miss], d[miss], s[miss]
    junk = torch.full((len(om), 3), 5.5, dtype=torch.float32, device="cuda:0")
    r = c.ds.raytrace(om, dm, seeds=sm, samples=8, k_range=(2, 5), sums=junk, want_rgb=True)
    torch.cuda.synchronize()
    assert (ibits(r.sum.cpu().numpy()) == 0).all() and (ibits(r.avg.cpu().numpy()) == 0).all() and (r.rgb.cpu().numpy() == 0).all()


# ---- 5. batch independence and chunks --------------------------------------------------------------------------------
def test_permuted_batches_single_rays_chunks_and_the_empty_batch(sqt, bright):
    import torch
    c = bright
    o, d, s = all_rays(c)
    try:
        set_options(c.ds)
        base = raytrace(c.ds, o, d, s, samples=2, want_rgb=True)
        perm = np.random.default_rng(5).permutation(len(o))
        got = raytrace(c.ds, o[perm], d[perm], s[perm], samples=2, want_rgb=True)
        for g, b in zip(got, base):
            assert np.array_equal(g.view(np.uint8), b[perm].view(np.uint8))
        for i in (0, 1, N_FAMILY + 7, 2 * N_FAMILY + 3, 3 * N_FAMILY, 3 * N_FAMILY + 1, 3 * N_FAMILY + 2, len(o) - 1):
            one = raytrace(c.ds, o[i:i + 1], d[i:i + 1], s[i:i + 1], samples=2, want_rgb=True)
            for g, b in zip(one, base):
                assert np.array_equal(g.view(np.uint8), b[i:i + 1].view(np.uint8)), i
        for opts in ({}, {"resident": 0}, {"variant": 1}):
            set_options(c.ds, slots=len(o) // 5 - 17, **opts)        # the wavefront forms: 6 chunks, the last one short
            got = raytrace(c.ds, o, d, s, samples=2, want_rgb=True)
            for g, b in zip(got, base):
                assert np.array_equal(g.view(np.uint8), b.view(np.uint8)), opts
            # the chunks do run: with one sample a chunk is one sample batch of two trace launches (a one-chunk query: 2 launches); the
            # per-lane form is one launch of one kernel whatever `slots` says
            c.ds.reset_timing()
            c.ds.enable_timing(True)
            raytrace(c.ds, o, d, s, samples=1)
            launches = c.ds.kernel_timing()[1]
            c.ds.enable_timing(False)
            c.ds.reset_timing()
            assert launches == (1 if opts.get("variant") == 1 else 6 * 2), (opts, launches)
    finally:
        set_options(c.ds)
    e = c.ds.raytrace(np.zeros((0, 3), f32), np.zeros((0, 3), f32), seeds=np.zeros(0, np.int64), want_rgb=True)
    assert e.sum.shape == (0, 3) and e.avg.shape == (0, 3) and e.rgb.shape == (0, 3)
    assert c.ds.raycast(np.zeros((0, 3), f32), np.zeros((0, 3), f32)).shape == (0, 3)
    assert sqt.lib().sq_raytrace_rays_device(c.ds._h, None, None, None, 0, 0, 1, None, None, None, None) == 0
    assert sqt.lib().sq_raycast_rays_device(c.ds._h, None, None, 0, None, None) == 0
    torch.cuda.synchronize()


# ---- 6. tall trees ---------------------------------------------------------------------------------------------------
def test_tall_tree_per_lane_form_equals_the_oracle_and_the_default_form_is_refused(sqt, O, shipped):
    import torch
    c = shipped
    cam = sqt.load_camera(os.path.join(DATA, "camera"))
    co, cd = (t.cpu().numpy().reshape(-1, 3) for t in c.ds.camera_rays(cam, 32, 24))
    axis, side = TP.near_side(cd)
    height = 200                                              # 2-byte words: the per-lane kernel takes it, the wavefront form does not
    ps = TP.full_stack(c.bih, height, axis, side)
    assert ps.height == height
    n = 1500
    o = np.concatenate([co] + [c.fam[k][0][:n] for k in FAMILIES])
    d = np.concatenate([cd] + [c.fam[k][1][:n] for k in FAMILIES])
    s = np.concatenate([np.arange(len(co), dtype=np.int64) * 7] + [c.seeds[k][:n] for k in FAMILIES])
    with np.errstate(all="ignore"):                           # the padding is transparent: the oracle's radiance on the unpadded scene
        want = (f32(0) + np.concatenate([oracle_raytrace(O, c.ob, co, cd, s[:len(co)])] + [c.exp[k][:n] for k in FAMILIES])).astype(f32)
    assert (want != 0).any(-1).sum() > 300
    ds = sqt.DeviceScene(ps, 0)
    try:
        for cull in (0, 1):
            set_options(ds, variant=1, cull=cull)
            got = raytrace(ds, o, d, s)[0]
            assert nan_eq(got, want).all(), (cull, int((~nan_eq(got, want)).any(-1).sum()))
            assert ds.last_plan()["trace_form"] == "per_pixel" and ds.last_plan()["height"] == height
        set_options(ds)
        sums = torch.full((len(o), 3), 7.5, dtype=torch.float32, device="cuda:0")
        avg = torch.full((len(o), 3), -3.25, dtype=torch.float32, device="cuda:0")
        rgb = torch.full((len(o), 3), 77, dtype=torch.uint8, device="cuda:0")
        to, td, ts = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda(), torch.from_numpy(s).cuda()
        rc = sqt.lib().sq_raytrace_rays_device(ds._h, to.data_ptr(), td.data_ptr(), ts.data_ptr(), len(o), 0, 1, sums.data_ptr(),
                                               avg.data_ptr(), rgb.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc != 0 and f"BIH height {height} needs" in sqt.lib().sq_last_error().decode()
        with pytest.raises(sqt.SquiglyError, match=f"BIH height {height} needs"):
            ds.raytrace(o, d, seeds=s)
        torch.cuda.synchronize()
        assert (sums == 7.5).all() and (avg == -3.25).all() and (rgb == 77).all()
        assert ds.last_plan()["launched"] == 0
    finally:
        ds.close()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------
def test_refusals_leave_every_buffer_as_it_was(sqt, shipped):
    import torch
    c = shipped
    ds = c.ds
    set_options(ds)
    L = sqt.lib()
    n = 1000
    dev = "cuda:0"
    o = torch.from_numpy(c.fam["to_light"][0][:n]).to(dev)
    d = torch.from_numpy(c.fam["to_light"][1][:n]).to(dev)
    sd = torch.from_numpy(c.seeds["to_light"][:n]).to(dev)
    big = torch.full((n * 3 + 64,), 1.25, dtype=torch.float32, device=dev)
    sm = torch.full((n, 3), 2.5, dtype=torch.float32, device=dev)
    av = torch.full((n, 3), -1.5, dtype=torch.float32, device=dev)
    rg = torch.full((n, 3), 99, dtype=torch.uint8, device=dev)
    bufs = (o, d, sd, sm, av, rg, big)
    snap = [t.clone() for t in bufs]
    p = lambda t: t.data_ptr()                                  # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = dict(org=p(o), dir=p(d), seed=p(sd), n=n, k0=0, k1=2, sum=p(sm), avg=p(av), rgb=p(rg))
    cases = {
        "null org": dict(org=None), "null dir": dict(dir=None), "null seed": dict(seed=None), "null sum": dict(sum=None),
        "n < 0": dict(n=-5), "k_begin < 0": dict(k0=-1), "empty range": dict(k0=2, k1=2), "reversed range": dict(k0=3, k1=1),
        "org = dir": dict(dir=p(o)),                              # two inputs
        "sum over org": dict(sum=p(o) + 12 * (n - 1)),             # an input over an output
        "avg over dir": dict(avg=p(d) + 4),
        "rgb in seed": dict(rgb=p(sd) + 8 * n - 1),
        "sum = avg": dict(avg=p(sm)),                             # two outputs
        "avg over rgb": dict(avg=p(big), rgb=p(big) + 12 * n - 3),
        "seed over sum": dict(seed=p(big) + 8, sum=p(big)),
    }
    for what, change in cases.items():
        a = {**good, **change}
        rc = L.sq_raytrace_rays_device(ds._h, a["org"], a["dir"], a["seed"], a["n"], a["k0"], a["k1"], a["sum"], a["avg"], a["rgb"], st)
        assert rc != 0, what
        assert len(L.sq_last_error()) > 0, what
    cast_cases = {"null org": (None, p(d), n, p(sm)), "null dir": (p(o), None, n, p(sm)), "null rad": (p(o), p(d), n, None),
                  "n < 0": (p(o), p(d), -1, p(sm)), "org = dir": (p(o), p(o), n, p(sm)), "rad over dir": (p(o), p(d), n, p(d) + 12 * (n - 1))}
    for what, args in cast_cases.items():
        assert L.sq_raycast_rays_device(ds._h, *args, st) != 0, what
        assert len(L.sq_last_error()) > 0, what
    torch.cuda.synchronize()
    for a, b in zip(bufs, snap):
        assert torch.equal(a, b)
    # adjacent, non-overlapping ranges are fine
    buf = torch.empty(n * 9, dtype=torch.float32, device=dev)
    buf[:3 * n] = o.reshape(-1)
    buf[3 * n:6 * n] = d.reshape(-1)
    assert L.sq_raytrace_rays_device(ds._h, p(buf), p(buf) + 12 * n, p(sd), n, 0, 2, p(buf) + 24 * n, None, None, st) == 0
    want = raytrace(ds, o, d, sd, samples=2)[0]
    torch.cuda.synchronize()
    assert np.array_equal(ibits(buf[6 * n:].cpu().numpy().reshape(n, 3)), ibits(want)) and want.any()


# ---- 8. raycast ------------------------------------------------------------------------------------------------------
def test_raycast_equals_the_oracles_cast_render_of_each_ray(O, shipped, bright):
    import torch
    for c in (shipped, bright):
        set_options(c.ds)
        n = 4000
        for k in ("free", "surface", "to_light"):
            o, d = c.fam[k][0][:n], c.fam[k][1][:n]
            want = oracle_raycast(O, c.ob, o, d)
            lit = float((want != 0).any(-1).mean())
            print(f"raycast, {k}: {lit:.3f} of the rays are lit")
            assert lit >= 0.20, (k, lit)
            for variant in (2, 1):
                set_options(c.ds, variant=variant)
                got = c.ds.raycast(o, d)
                torch.cuda.synchronize()
                got = got.cpu().numpy()
                assert nan_eq(got, want).all(), (k, variant, int((~nan_eq(got, want)).any(-1).sum()))
                assert c.ds.last_plan()["trace_form"] == "per_pixel" and c.ds.last_plan()["launched"] == 1
        set_options(c.ds)


@pytest.mark.parametrize("spp", (1, 3))
@pytest.mark.parametrize("shard", ((None, 0, 1), (2, 1, 3)))
def test_a_cast_frame_is_the_raycast_of_its_camera_rays(sqt, shipped, spp, shard):
    import torch
    ds = shipped.ds
    set_options(ds)
    cam = sqt.load_camera(os.path.join(DATA, "camera"))
    avg, _ = ds.render_rows(cam, spp, 64, 64, cast=True, shard=shard)
    c = ds.raycast(*ds.camera_rays(cam, 64, 64, shard=shard))
    torch.cuda.synchronize()
    c = c.cpu().numpy()
    with np.errstate(all="ignore"):
        want = ((f32(1) / f32(spp)) * fold([c] * spp)).astype(f32)
    got = avg.cpu().numpy()
    assert got.any()
    assert np.array_equal(ibits(got), ibits(want)), int((ibits(got) != ibits(want)).any(-1).sum())
    assert np.array_equal(ibits(got), ibits(cast_from_queries(ds, shipped.bih, cam, spp, 64, 64, shard)))


# ---- 9. the Python surface -------------------------------------------------------------------------------------------
def test_python_surface_shapes_inputs_and_outputs(sqt, bright):
    import torch
    c = bright
    ds = c.ds
    set_options(ds)
    o, d, s = c.fam["to_light"][0][:60], c.fam["to_light"][1][:60], c.seeds["to_light"][:60]
    flat = raytrace(ds, o, d, s, samples=3, want_rgb=True)
    assert flat[0].any()
    r = ds.raytrace(o.reshape(3, 4, 5, 3), torch.from_numpy(d.reshape(3, 4, 5, 3)), seeds=s.reshape(3, 4, 5), samples=3, want_rgb=True)
    torch.cuda.synchronize()
    assert r.sum.shape == r.avg.shape == r.rgb.shape == (3, 4, 5, 3)
    assert r.sum.dtype == torch.float32 and r.avg.dtype == torch.float32 and r.rgb.dtype == torch.uint8 and r.sum.is_cuda
    for g, e in zip(r, flat):
        assert np.array_equal(g.cpu().numpy().reshape(e.shape).view(np.uint8), e.view(np.uint8))
    one = ds.raytrace(o[0], d[0], seeds=np.int64(s[0]), samples=3)       # a single ray [3]: scalar leading shape
    torch.cuda.synchronize()
    assert one.sum.shape == (3,) and one.rgb is None and np.array_equal(ibits(one.sum.cpu().numpy()), ibits(flat[0][0]))
    # float64 input is rounded to float32 first; lists and CUDA tensors work
    o64 = o.astype(np.float64) + 1e-12
    g = raytrace(ds, o64, d.tolist(), s.tolist(), samples=3)
    w = raytrace(ds, torch.from_numpy(o64.astype(f32)).cuda(), torch.from_numpy(d).cuda(), torch.from_numpy(s).cuda(), samples=3)
    assert np.array_equal(ibits(g[0]), ibits(w[0])) and np.array_equal(ibits(g[0]), ibits(flat[0]))
    r = ds.raytrace(o, d, seeds=s, samples=3, want_avg=False)
    assert r.avg is None and r.rgb is None
    # seeds=None: samples * i in row-major order
    a = raytrace(ds, o.reshape(6, 10, 3), d.reshape(6, 10, 3), None, samples=3)
    b = raytrace(ds, o, d, 3 * np.arange(60, dtype=np.int64), samples=3)
    assert np.array_equal(ibits(a[0].reshape(60, 3)), ibits(b[0]))
    # sums is reused, not replaced
    sums = torch.empty(60, 3, dtype=torch.float32, device="cuda:0")
    r = ds.raytrace(o, d, seeds=s, samples=3, k_range=(0, 1), sums=sums)
    r = ds.raytrace(o, d, seeds=s, samples=3, k_range=(1, 3), sums=r.sum)
    torch.cuda.synchronize()
    assert r.sum is sums and np.array_equal(ibits(sums.cpu().numpy()), ibits(flat[0]))
    assert np.array_equal(ibits(r.avg.cpu().numpy()), ibits(flat[1]))
    rad = ds.raycast(o.reshape(3, 20, 3), d.reshape(3, 20, 3).tolist())
    assert rad.shape == (3, 20, 3) and rad.dtype == torch.float32 and rad.is_cuda
    for bad in ((o[:, :2], d[:, :2]), (o, d[:59]), (o.reshape(-1), d.reshape(-1))):
        with pytest.raises(sqt.SquiglyError):
            ds.raytrace(*bad)
        with pytest.raises(sqt.SquiglyError):
            ds.raycast(*bad)
    for kw in ({"seeds": s[:59]}, {"seeds": s.astype(np.float32)}, {"k_range": (1, 2)}, {"k_range": (2, 2)}, {"samples": 0},
               {"sums": torch.empty(59, 3, device="cuda:0")}, {"sums": torch.empty(60, 3, dtype=torch.float64, device="cuda:0")},
               {"sums": torch.empty(60, 3)}):
        with pytest.raises(sqt.SquiglyError):
            ds.raytrace(o, d, **kw)
