"""Ray queries on a resident scene (sq_intersect_rays_device, sq_camera_rays_device, DeviceScene.intersect / camera_rays): every
ray's (tri, dist, point) is bit for bit the oracle's intersectBIH (src/BIH.hs:101-141), in every trace form and option, for rays far
from the camera and bounce rays the frames trace: free space, axis-aligned, on split planes, non-finite and degenerate."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

import render_options as RO
import tree_padding as TP
from bitcmp import ibits
from conftest import DATA, ROOT
from ray_oracle import FAMILIES, N_FAMILY, cast_from_queries, check_hits, make_families, oracle_hits, query
from render_options import SCENE_FORMS

pytestmark = pytest.mark.gpu
f32 = np.float32
set_options = functools.partial(RO.set_options, table=RO.RAY_QUERY)


# ---- fixtures ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(sqt, O):
    bih = sqt.BIH(sqt.Mesh.from_obj(os.path.join(DATA, "scene.obj"), DATA))
    ob = O.BIH(O.tris_from_obj(os.path.join(DATA, "scene.obj"), DATA))
    fam = make_families(bih, 1)
    exp = {k: oracle_hits(ob, *fam[k]) for k in FAMILIES}
    for k in FAMILIES:                                        # every family has hits and misses
        assert (exp[k][0] >= 0).any() and (exp[k][0] < 0).any(), k
    ds = sqt.DeviceScene(bih, 0)
    yield bih, ob, ds, fam, exp
    ds.close()


@pytest.fixture(scope="module")
def blob(sqt, O):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_scenes as G
    obj, sq, _ = G.blob_scene(6)
    bih = sqt.BIH(sqt.Mesh.from_text(obj.encode() if isinstance(obj, str) else obj, sq.encode() if isinstance(sq, str) else sq))
    assert bih.scene.n_tris == 81920 + 12                    # the blob and the room
    ob = O.BIH(O.tris_from_text(obj.encode() if isinstance(obj, str) else obj, sq.encode() if isinstance(sq, str) else sq))
    fam = make_families(bih, 2)
    exp = {k: oracle_hits(ob, *fam[k]) for k in FAMILIES}
    ds = sqt.DeviceScene(bih, 0)
    yield bih, ds, fam, exp
    ds.close()


def all_rays(fam):
    return np.concatenate([fam[k][0] for k in FAMILIES]), np.concatenate([fam[k][1] for k in FAMILIES])


def check_families(ds, fam, exp, what):
    o, d = all_rays(fam)
    got = query(ds, o, d)
    for i, k in enumerate(FAMILIES):
        s = slice(i * N_FAMILY, (i + 1) * N_FAMILY)
        check_hits(tuple(g[s] for g in got), exp[k], what + (k,))
    return got


# ---- 1. against the oracle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts, form", SCENE_FORMS, ids=[f"{f}-{'-'.join(f'{k}{v}' for k, v in o.items()) or 'default'}" for o, f in SCENE_FORMS])
def test_scene_queries_equal_the_oracle_in_every_form(scene, opts, form):
    _, _, ds, fam, exp = scene
    try:
        for cull in (0, 1):
            set_options(ds, cull=cull, **opts)
            check_families(ds, fam, exp, (form, opts, cull))
            plan = ds.last_plan()
            assert plan["trace_form"] == form and plan["launched"] == 1 and plan["primary_form"] == "none", plan
    finally:
        set_options(ds)


@pytest.mark.parametrize("opts", ({"variant": 1}, {}, {"pool": 0}), ids=("variant1", "default", "pool0"))
def test_blob_queries_equal_the_oracle_with_4_byte_stack_words(blob, opts):
    _, ds, fam, exp = blob
    try:
        set_options(ds, **opts)
        check_families(ds, fam, exp, ("blob", opts))
        plan = ds.last_plan()
        assert plan["stack_word_bytes"] == 4 and plan["launched"] == 1, plan
        want = {"variant": "per_pixel"} if opts.get("variant") == 1 else None
        if want:
            assert plan["trace_form"] == "per_pixel"
        elif opts.get("pool") == 0:
            assert plan["trace_form"] == "streaming_plain", plan
        else:
            assert plan["trace_form"] in ("streaming_six_wave", "streaming_plain"), plan
    finally:
        set_options(ds)


# ---- 2. batch independence -------------------------------------------------------------------------------------------
def test_permuted_rays_give_permuted_results_and_one_ray_equals_its_entry(scene):
    _, _, ds, fam, _ = scene
    set_options(ds)
    o, d = all_rays(fam)
    base = query(ds, o, d)
    perm = np.random.default_rng(5).permutation(len(o))
    got = query(ds, o[perm], d[perm])
    for g, b in zip(got, base):
        assert np.array_equal(g.view(np.int32), b[perm].view(np.int32))
    for i in (0, 1, N_FAMILY + 7, 2 * N_FAMILY + 3, 3 * N_FAMILY, 3 * N_FAMILY + 1, 3 * N_FAMILY + 2, len(o) - 1):
        one = query(ds, o[i:i + 1], d[i:i + 1])
        for g, b in zip(one, base):
            assert np.array_equal(g.view(np.int32), b[i:i + 1].view(np.int32)), i


# ---- 3. chunks -------------------------------------------------------------------------------------------------------
def test_chunked_queries_equal_one_chunk_and_n0_is_a_no_op(sqt, scene):
    import torch
    _, _, ds, fam, _ = scene
    o, d = all_rays(fam)
    try:
        set_options(ds)
        one = query(ds, o, d)
        for opts in ({}, {"resident": 0}):
            set_options(ds, slots=len(o) // 5 - 17, **opts)      # 6 chunks, the last one short
            got = query(ds, o, d)
            for g, b in zip(got, one):
                assert np.array_equal(g.view(np.int32), b.view(np.int32)), opts
    finally:
        set_options(ds)
    e = ds.intersect(np.zeros((0, 3), f32), np.zeros((0, 3), f32))
    assert e.tri.shape == (0,) and e.dist.shape == (0,) and e.point.shape == (0, 3)
    assert sqt.lib().sq_intersect_rays_device(ds._h, None, None, 0, None, None, None, None) == 0
    torch.cuda.synchronize()


# ---- 4. tall trees ---------------------------------------------------------------------------------------------------
def test_tall_tree_per_lane_form_equals_the_mirror_and_the_default_form_is_refused(sqt, scene):
    import torch
    bih, _, _, fam, _ = scene
    cam_o, cam_d = camera_rays_np(sqt, bih, 32, 24)
    axis, side = TP.near_side(cam_d)
    height = 200                                              # 2-byte words: the per-lane kernel takes it, the wavefront form does not
    ps = TP.full_stack(bih, height, axis, side)
    assert ps.height == height
    o = np.concatenate([cam_o, fam["free"][0][:1500], fam["degenerate"][0][:500]])
    d = np.concatenate([cam_d, fam["free"][1][:1500], fam["degenerate"][1][:500]])
    m = TP.Mirror(ps.nodes, ps.tris, bih.scene.root.lo[:], bih.scene.root.hi[:])
    etri, edist, ept = m.intersect(o, d)
    assert (etri >= 0).sum() > 500
    ds = sqt.DeviceScene(ps, 0)
    try:
        for cull in (0, 1):
            set_options(ds, variant=1, cull=cull)
            check_hits(query(ds, o, d), (etri, edist, ept), ("tall", cull))
            assert ds.last_plan()["trace_form"] == "per_pixel" and ds.last_plan()["height"] == height
        set_options(ds)
        tri = torch.full((len(o),), 12345, dtype=torch.int32, device="cuda:0")
        dist = torch.full((len(o),), 7.5, dtype=torch.float32, device="cuda:0")
        pt = torch.full((len(o), 3), -3.25, dtype=torch.float32, device="cuda:0")
        with pytest.raises(sqt.SquiglyError, match=f"BIH height {height} needs"):
            ds.intersect(o, d, out=sqt.Hits(tri, dist, pt))
        torch.cuda.synchronize()
        assert (tri == 12345).all() and (dist == 7.5).all() and (pt == -3.25).all()
        assert ds.last_plan()["launched"] == 0
    finally:
        ds.close()


# ---- 5. refusals -----------------------------------------------------------------------------------------------------
def test_refusals_leave_every_buffer_as_it_was(sqt, scene):
    import torch
    _, _, ds, fam, _ = scene
    set_options(ds)
    L = sqt.lib()
    n = 1000
    dev = "cuda:0"
    o = torch.from_numpy(fam["free"][0][:n]).to(dev)
    d = torch.from_numpy(fam["free"][1][:n]).to(dev)
    big = torch.zeros(n * 3 + 64, dtype=torch.float32, device=dev)
    tri = torch.full((n,), 777, dtype=torch.int32, device=dev)
    dist = torch.full((n,), 2.5, dtype=torch.float32, device=dev)
    pt = torch.full((n, 3), -1.5, dtype=torch.float32, device=dev)
    snap = [t.clone() for t in (o, d, tri, dist, pt, big)]
    p = lambda t: t.data_ptr()                                  # noqa: E731
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    cases = {
        "null org": (None, p(d), n, p(tri), p(dist), p(pt)),
        "null dir": (p(o), None, n, p(tri), p(dist), p(pt)),
        "null tri": (p(o), p(d), n, None, p(dist), p(pt)),
        "n < 0": (p(o), p(d), -5, p(tri), p(dist), p(pt)),
        "org = dir": (p(o), p(o), n, p(tri), p(dist), p(pt)),
        "dist in tri": (p(o), p(d), n, p(tri), p(tri) + 4, p(pt)),
        "point over org": (p(o), p(d), n, p(tri), p(dist), p(o) + 12 * (n - 1)),
        "point over dist": (p(o), p(d), n, p(tri), p(big), p(big) + 8),
        "dir over point": (p(o), p(big) + 4, n, p(tri), p(dist), p(big)),
    }
    for what, args in cases.items():
        assert L.sq_intersect_rays_device(ds._h, *args, s) != 0, what
        assert len(L.sq_last_error()) > 0, what
    torch.cuda.synchronize()
    for a, b in zip((o, d, tri, dist, pt, big), snap):
        assert torch.equal(a, b)
    # adjacent, non-overlapping ranges are fine
    buf = torch.empty(n * 6, dtype=torch.float32, device=dev)
    buf[:3 * n] = o.reshape(-1)
    buf[3 * n:] = d.reshape(-1)
    assert L.sq_intersect_rays_device(ds._h, p(buf), p(buf) + 12 * n, n, p(tri), None, None, s) == 0
    want = query(ds, o, d)
    torch.cuda.synchronize()
    assert np.array_equal(tri.cpu().numpy(), want[0])


# ---- 6. camera rays --------------------------------------------------------------------------------------------------
def camera_rays_np(sqt, bih, w, h):
    """Primary rays of the product's data/camera as flat numpy arrays (a fresh scene, so it works without the module fixture)."""
    ds = sqt.DeviceScene(bih, 0)
    try:
        o, d = ds.camera_rays(sqt.load_camera(os.path.join(DATA, "camera")), w, h)
        return o.cpu().numpy().reshape(-1, 3), d.cpu().numpy().reshape(-1, 3)
    finally:
        ds.close()


@pytest.mark.parametrize("text, w, h, shard", [("rotated", 23, 37, (None, 0, 1)), ("rotated", 23, 37, (2, 1, 3)), ("camera", 64, 64, (None, 0, 1))])
def test_camera_rays_equal_make_ray(sqt, O, scene, text, w, h, shard):
    _, _, ds, _, _ = scene
    t = open(os.path.join(DATA, "camera")).read().encode() if text == "camera" else b"0 7 0.75\n1.4 0.15 0.2\n"
    cp, co = sqt.camera_from_text(t), O.camera_from_text(t)
    o, d = ds.camera_rays(cp, w, h, shard=shard)
    o, d = o.cpu().numpy(), d.cpu().numpy()
    rb, si, ns = shard
    sh = sqt.Shard(w if rb is None else rb, si, ns)
    rows = sqt.lib().sq_shard_rows(w, sh)
    assert o.shape == d.shape == (rows, h, 3)
    for j in range(rows):
        y = sqt.lib().sq_shard_global_row(j, sh)
        for x in range(h):
            eo, ed = O.make_ray(w, h, y, x, co)
            assert np.array_equal(ibits(o[j, x]), ibits(eo)) and np.array_equal(ibits(d[j, x]), ibits(ed)), (j, x)


# ---- 7. a cast frame rebuilt from two queries ------------------------------------------------------------------------
@pytest.mark.parametrize("spp", (1, 3))
@pytest.mark.parametrize("shard", ((None, 0, 1), (2, 1, 3)))
def test_cast_frame_equals_its_restatement_from_queries(sqt, scene, spp, shard):
    import torch
    bih, _, ds, _, _ = scene
    set_options(ds)
    cam = sqt.load_camera(os.path.join(DATA, "camera"))
    want = cast_from_queries(ds, bih, cam, spp, 64, 64, shard)
    avg, _ = ds.render_rows(cam, spp, 64, 64, cast=True, shard=shard)
    torch.cuda.synchronize()
    got = avg.cpu().numpy()
    assert got.any()
    assert np.array_equal(ibits(got), ibits(want)), int((ibits(got) != ibits(want)).any(-1).sum())


# ---- 8. misses are black ---------------------------------------------------------------------------------------------
def test_pixels_whose_camera_ray_misses_are_black(sqt, scene):
    import torch
    _, _, ds, _, _ = scene
    set_options(ds)
    cam = sqt.camera_from_text(b"0.4 6.2 1.1\n1.5707963267948966 0 -0.39\n")
    avg, _ = ds.render_rows(cam, 2, 48, 40)
    hits = ds.intersect(*ds.camera_rays(cam, 48, 40))
    torch.cuda.synchronize()
    miss = (hits.tri < 0).cpu().numpy()
    assert miss.any() and (~miss).any()
    assert (ibits(avg.cpu().numpy()[miss]) == 0).all()


# ---- 9. the Python surface -------------------------------------------------------------------------------------------
def test_python_surface_shapes_inputs_and_outputs(sqt, scene):
    import torch
    _, _, ds, fam, exp = scene
    set_options(ds)
    o, d = fam["surface"][0][:60], fam["surface"][1][:60]
    flat = query(ds, o, d)
    h = ds.intersect(o.reshape(3, 4, 5, 3), torch.from_numpy(d.reshape(3, 4, 5, 3)))
    torch.cuda.synchronize()
    assert h.tri.shape == (3, 4, 5) and h.dist.shape == (3, 4, 5) and h.point.shape == (3, 4, 5, 3)
    assert h.tri.dtype == torch.int32 and h.dist.dtype == torch.float32 and h.tri.is_cuda
    assert np.array_equal(h.tri.cpu().numpy().reshape(-1), flat[0])
    assert np.array_equal(ibits(h.point.cpu().numpy().reshape(-1, 3)), ibits(flat[2]))
    one = ds.intersect(o[0], d[0])                             # a single ray [3]: scalar leading shape
    torch.cuda.synchronize()
    assert one.tri.shape == () and one.point.shape == (3,) and int(one.tri) == flat[0][0]
    # float64 input is rounded to float32 first; lists and CUDA tensors work
    o64 = o.astype(np.float64) + 1e-12
    g = query(ds, o64, d.tolist())
    w = query(ds, o64.astype(f32), d)
    for a, b in zip(g, w):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    h = ds.intersect(torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda(), want_dist=False, want_point=False)
    torch.cuda.synchronize()
    assert h.dist is None and h.point is None and np.array_equal(h.tri.cpu().numpy(), flat[0])
    out = sqt.Hits(torch.empty(60, dtype=torch.int32, device="cuda:0"), torch.empty(60, device="cuda:0"), torch.empty(60, 3, device="cuda:0"))
    r = ds.intersect(o, d, out=out)
    torch.cuda.synchronize()
    assert r.tri is out.tri and r.dist is out.dist and r.point is out.point
    assert np.array_equal(out.tri.cpu().numpy(), flat[0]) and np.array_equal(ibits(out.dist.cpu().numpy()), ibits(flat[1]))
    for bad in ((o[:, :2], d[:, :2]), (o, d[:59]), (o.reshape(-1), d.reshape(-1))):
        with pytest.raises(sqt.SquiglyError):
            ds.intersect(*bad)
    with pytest.raises(sqt.SquiglyError):
        ds.intersect(o, d, out=sqt.Hits(torch.empty(59, dtype=torch.int32, device="cuda:0"), None, None))
    with pytest.raises(sqt.SquiglyError):
        ds.intersect(o, d, out=sqt.Hits(torch.empty(60, dtype=torch.int64, device="cuda:0"), None, None))
