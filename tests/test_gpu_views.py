"""Many views in one call (sq_render_views_device, DeviceScene.render_views, render_views_rgb8 and the CLI's --views): view i of a
batched call is bit for bit the single-view frame of cams[i] and the oracle's image, in every kernel form, schedule and option.
Frames are small and odd (23 rows x 37 columns) so that the primary-ray tiles are padded at every view boundary."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import render_options as RO
from bitcmp import ibits
from conftest import DATA, ROOT
from render_options import OPTION_TUPLES, THREADS
from scenes import ROTATED, tall_u32 as _tall_u32

pytestmark = pytest.mark.gpu
set_options = functools.partial(RO.set_options, table=RO.VIEWS)
W, H, SPP = 23, 37, 3

CAMERA = open(os.path.join(DATA, "camera")).read().encode()
CAM_TEXTS = {
    "camera": CAMERA,
    "moved": b"0.4 6.2 1.1\n1.5707963267948966 0 -0.09817477042468103\n",
    "rotated": ROTATED,
    "miss": b"0 7 0.75\n-1.5707963267948966 0 0\n",               # looks away from the scene: every primary ray misses
}
FIVE = ("camera", "moved", "rotated", "miss", "camera")               # the last one duplicates view 0


def cameras(sqt, O, texts):
    """Product and oracle cameras of the same texts; their words must be equal."""
    cp = [sqt.camera_from_text(t) for t in texts]
    co = [O.camera_from_text(t) for t in texts]
    for p, o in zip(cp, co):
        pos, rot = O.camera_arrays(o)
        assert np.array_equal(np.array(p.pos[:], np.float32).view(np.int32), pos.view(np.int32))
        assert np.array_equal(np.array(p.rot[:], np.float32).view(np.int32), rot.view(np.int32))
    return cp, co


def singles(ds, cams, n, w, h, cast=False, shard=(None, 0, 1)):
    import torch
    out = [ds.render_rows(c, n, w, h, cast=cast, shard=shard) for c in cams]
    torch.cuda.synchronize()
    return [(a.cpu(), r.cpu()) for a, r in out]


def views(ds, cams, n, w, h, **kw):
    import torch
    a, r = ds.render_views(cams, n, w, h, **kw)
    torch.cuda.synchronize()
    return a.cpu(), r.cpu()


def assert_views_equal(got, want, what):
    a, r = got
    assert a.shape[0] == r.shape[0] == len(want), what
    for i, (wa, wr) in enumerate(want):
        assert np.array_equal(ibits(a[i]), ibits(wa)), (what, i, "avg")
        assert np.array_equal(r[i].numpy(), np.asarray(wr.numpy() if hasattr(wr, "numpy") else wr)), (what, i, "rgb")


@pytest.fixture(scope="module")
def dev(sqt, product_scene):
    assert sqt.device_count() >= 1, "no HIP device: the product has no CPU fallback"
    bih, _, _ = product_scene
    ds = sqt.DeviceScene(bih, 0)
    yield ds
    ds.close()


@pytest.fixture(scope="module")
def five(sqt, O, oracle_scene):
    """Product cameras of FIVE and the oracle's (avg, rgb) of every view, path-traced and cast."""
    ob, _, _ = oracle_scene
    cp, co = cameras(sqt, O, [CAM_TEXTS[k] for k in FIVE])
    exp = {cast: [ob.render(c, SPP, W, H, cast=cast, threads=THREADS)[:2] for c in co] for cast in (False, True)}
    for cast in (False, True):
        assert not exp[cast][3][0].any() and not exp[cast][3][1].any()       # the miss view is black
        assert exp[cast][0][1].any() and exp[cast][1][1].any() and exp[cast][2][1].any()
    return cp, exp


# ---- 1. five views against single calls and the oracle ---------------------------------------------------------------
@pytest.mark.parametrize("opts", OPTION_TUPLES)
def test_five_views_equal_single_calls_and_the_oracle(sqt, dev, five, opts):
    import torch
    cams, exp = five
    try:
        for cull in (0, 1):
            set_options(dev, cull=cull, **dict(zip(("variant", "resident", "profile", "overlap", "primary_pooled"), opts)))
            for cast in (False, True):
                what = (opts, cull, cast)
                got = views(dev, cams, SPP, W, H, cast=cast)
                assert_views_equal(got, singles(dev, cams, SPP, W, H, cast=cast), what + ("single",))
                assert_views_equal(got, [(torch.from_numpy(a), torch.from_numpy(r)) for a, r in exp[cast]], what + ("oracle",))
                assert np.array_equal(ibits(got[0][4]), ibits(got[0][0])) and torch.equal(got[1][4], got[1][0])
                sums = torch.full((len(cams), W, H, 3), float("nan"), dtype=torch.float32, device="cuda:0")
                got2 = views(dev, cams, SPP, W, H, cast=cast, sums=sums)
                assert_views_equal(got2, [(got[0][i], got[1][i]) for i in range(len(cams))], what + ("with sums",))
                assert (ibits(sums[3]) == 0).all(), what                    # the miss view's sums are +0
    finally:
        set_options(dev)


# ---- 2. view order ---------------------------------------------------------------------------------------------------
def test_view_order_permutes_the_images(dev, five):
    cams, _ = five
    set_options(dev)
    a, b, c = cams[0], cams[1], cams[2]
    x = views(dev, [a, b, c], SPP, W, H)
    y = views(dev, [c, a, b], SPP, W, H)
    for i, j in ((0, 1), (1, 2), (2, 0)):
        assert np.array_equal(ibits(x[0][i]), ibits(y[0][j])) and np.array_equal(x[1][i].numpy(), y[1][j].numpy()), (i, j)


# ---- 3. one view -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts", [{}, {"variant": 1}, {"primary_pooled": 1}, {"overlap": 2}])
def test_one_view_is_render_rows_with_the_same_plan(dev, five, opts):
    cams, _ = five
    set_options(dev, **opts)
    try:
        want = singles(dev, cams[:1], SPP, W, H)
        plan = dev.last_plan()
        got = views(dev, cams[:1], SPP, W, H)
        assert tuple(got[0].shape) == (1, W, H, 3)
        assert_views_equal(got, want, opts)
        assert dev.last_plan() == plan
    finally:
        set_options(dev)


# ---- 4. shards -------------------------------------------------------------------------------------------------------
def test_shards_reassemble_to_whole_views(dev, five):
    from importlib import import_module
    d = import_module("squigly-trace_amd.dist")
    cams, _ = five
    set_options(dev)
    whole = views(dev, cams, SPP, W, H)
    seen = np.zeros(W, bool)
    for r in range(3):
        part = views(dev, cams, SPP, W, H, shard=(2, r, 3))
        rows = d.shard_rows(W, 2, r, 3)
        assert part[0].shape[:2] == (len(cams), len(rows))
        assert np.array_equal(ibits(part[0]), ibits(whole[0][:, rows])), r
        assert np.array_equal(part[1].numpy(), whole[1][:, rows].numpy()), r
        seen[rows] = True
    assert seen.all()


# ---- 5. many batches, two tracks -------------------------------------------------------------------------------------
@pytest.mark.parametrize("overlap", [0, 1, 2])
def test_many_batches_and_two_tracks(sqt, product_scene, dev, five, overlap):
    cams, _ = five
    n = 7
    set_options(dev)
    want = singles(dev, cams, n, W, H)
    ds = sqt.DeviceScene(product_scene[0], 0)                          # a fresh workspace: it holds only what `slots` asks for
    try:
        set_options(ds, overlap=overlap, slots=len(cams) * W * H * 2)  # two samples per batch (one per track when overlapped)
        assert_views_equal(views(ds, cams, n, W, H), want, overlap)
    finally:
        ds.close()


# ---- 6. ranges -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts", [{}, {"variant": 1}, {"overlap": 1}])
def test_ranges_equal_one_call_and_single_view_ranges(dev, five, opts):
    import torch
    cams, _ = five
    set_options(dev, **opts)
    try:
        whole = views(dev, cams, SPP, W, H)
        sums = torch.empty((len(cams), W, H, 3), dtype=torch.float32, device="cuda:0")
        dev.render_views(cams, SPP, W, H, k_begin=0, k_end=1, sums=sums)
        got = views(dev, cams, SPP, W, H, k_begin=1, k_end=SPP, sums=sums)
        assert_views_equal(got, [(whole[0][i], whole[1][i]) for i in range(len(cams))], opts)
        for i, c in enumerate(cams):
            s1 = torch.empty((W, H, 3), dtype=torch.float32, device="cuda:0")
            dev.render_rows_range(c, SPP, W, H, 0, SPP, s1)
            torch.cuda.synchronize()
            assert np.array_equal(ibits(sums[i]), ibits(s1)), (opts, i)
    finally:
        set_options(dev)


# ---- 7. many small views ---------------------------------------------------------------------------------------------
def test_64_small_views_on_distinct_cameras(sqt, dev):
    texts = [f"{0.05 * (i % 8) - 0.175:.3f} {1.8 - 0.04 * (i // 8):.3f} 0.5\n{1.5707963267948966 + 0.02 * (i - 32):.6f} 0 "
             f"-0.09817477042468103\n".encode() for i in range(64)]          # inside the room, yaw swept
    cams = [sqt.camera_from_text(t) for t in texts]
    set_options(dev)
    got = views(dev, cams, 2, 8, 8)
    want = singles(dev, cams, 2, 8, 8)
    assert_views_equal(got, want, "64 views")
    assert len({bytes(ibits(a)) for a in got[0]}) > 16                 # the cameras do differ (the oracle: 22 distinct images)


# ---- 8. 4-byte stack words -------------------------------------------------------------------------------------------
def test_views_with_4_byte_stack_words(sqt, O, product_scene, oracle_scene):
    import tree_padding as TP
    bih0, _, _ = product_scene
    ob, _, _ = oracle_scene
    texts = [CAM_TEXTS[k] for k in ("camera", "moved", "rotated")]
    cp, co = cameras(sqt, O, texts)
    axis, side = TP.near_side([O.make_ray(W, H, y, x, co[0])[1] for y in range(W) for x in range(H)])
    ps = _tall_u32(bih0, bih0.height + 9, axis, side)
    assert ps.n_branches == 0x9000
    exp = [ob.render(c, SPP, W, H, threads=THREADS)[:2] for c in co]
    ds = sqt.DeviceScene(ps, 0)
    try:
        for opts in ({}, {"variant": 1}):
            set_options(ds, **opts)
            got = views(ds, cp, SPP, W, H)
            assert ds.last_plan()["stack_word_bytes"] == 4
            for i, (a, r) in enumerate(exp):
                assert np.array_equal(ibits(got[0][i]), ibits(a)), (opts, i)
                assert np.array_equal(got[1][i].numpy(), r), (opts, i)
    finally:
        ds.close()


# ---- 9. refusals -----------------------------------------------------------------------------------------------------
def test_refusals_leave_every_buffer_untouched(sqt, product_scene, dev, five):
    import torch
    import tree_padding as TP
    bih, _, _ = product_scene
    cams, _ = five
    set_options(dev)
    L = sqt.lib()
    w, h, n, nv = 16, 12, 4, 3
    table = (sqt.Camera * nv)(*cams[:nv])
    sh = sqt.Shard(w, 0, 1)
    sums = torch.full((nv, w, h, 3), 7.25, dtype=torch.float32, device="cuda:0")
    avg = torch.full((nv, w, h, 3), -3.5, dtype=torch.float32, device="cuda:0")
    rgb = torch.full((nv, w, h, 3), 123, dtype=torch.uint8, device="cuda:0")
    keep = (sums.clone(), avg.clone(), rgb.clone())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    S, A, R = sums.data_ptr(), avg.data_ptr(), rgb.data_ptr()

    def call(ds_h, n_views=nv, cams_p=table, kb=0, ke=n, s_ptr=S, a_ptr=A, r_ptr=R, shard=sh, ww=w, hh=h):
        return L.sq_render_views_device(ds_h, cams_p, n_views, n, ww, hh, 0, shard, kb, ke, s_ptr, a_ptr, r_ptr, stream)

    cases = {
        "n_views 0": dict(n_views=0),
        "n_views < 0": dict(n_views=-2),
        "cams NULL": dict(cams_p=None),
        "pixels > INT32_MAX": dict(n_views=(2 ** 31 - 1) // (w * h) + 1),   # refused before the table or a buffer is read
        "k_begin < 0": dict(kb=-1),
        "k_end == k_begin": dict(kb=2, ke=2),
        "k_end > samples": dict(ke=n + 1),
        "d_sum NULL, part of the frame": dict(kb=1, s_ptr=None),
        "d_sum NULL, first part": dict(ke=n - 1, s_ptr=None),
        "d_sum == d_avg": dict(a_ptr=S),
        "no output buffer": dict(s_ptr=None, a_ptr=None, r_ptr=None),
        "bad shard": dict(shard=sqt.Shard(2, 3, 3)),
    }
    for what, kw in cases.items():
        assert call(dev._h, **kw) != 0, what
        assert len(L.sq_last_error()) > 0, what
    assert call(dev._h, n_views=46341, ww=46341, hh=1, shard=sqt.Shard(46341, 0, 1)) != 0  # 46341^2 > 2^31 - 1
    assert b"exceed" in L.sq_last_error()
    for height, variant in ((200, 2), (400, 1), (400, 2)):
        ds = sqt.DeviceScene(TP.full_stack(bih, height, 0, TP.LEFT), 0)
        try:
            ds.set_option("variant", variant)
            assert call(ds._h, kb=1) != 0
            assert f"BIH height {height} needs".encode() in L.sq_last_error(), L.sq_last_error()
            assert ds.last_plan()["launched"] == 0
            torch.cuda.synchronize()
        finally:
            ds.close()
    with pytest.raises(ValueError):
        dev.render_views([], n, w, h)
    with pytest.raises(sqt.SquiglyError):
        dev.render_views(cams[:nv], n, w, h, sums=sums[:2])               # wrong shape
    torch.cuda.synchronize()
    for got, want in zip((sums, avg, rgb), keep):
        assert torch.equal(got, want)


# ---- 10. workspace reuse ---------------------------------------------------------------------------------------------
def test_workspace_and_camera_table_reuse(sqt, product_scene, five):
    bih, _, _ = product_scene
    cams, _ = five

    def fresh(fn):
        ds = sqt.DeviceScene(bih, 0)
        try:
            return fn(ds)
        finally:
            ds.close()
    many = [cams[i % 3] for i in range(70)]                              # more than one staging chunk of cameras
    ds = sqt.DeviceScene(bih, 0)
    try:
        a = views(ds, cams[:2], SPP, W, H)
        b = singles(ds, cams[2:3], SPP, W, H)
        c = views(ds, many, SPP, W, H)
    finally:
        ds.close()
    assert_views_equal(a, [(x, y) for x, y in zip(*fresh(lambda d: views(d, cams[:2], SPP, W, H)))], "first")
    assert_views_equal((b[0][0][None], b[0][1][None]), fresh(lambda d: singles(d, cams[2:3], SPP, W, H)), "single")
    want = fresh(lambda d: views(d, many, SPP, W, H))
    assert_views_equal(c, [(want[0][i], want[1][i]) for i in range(len(many))], "larger")
    assert np.array_equal(ibits(c[0][69]), ibits(c[0][0])) and np.array_equal(ibits(c[0][67]), ibits(a[0][1]))


# ---- 11. CLI ---------------------------------------------------------------------------------------------------------
def test_cli_views_write_one_png_per_camera(sqt, product_scene, tmp_path, monkeypatch):
    from importlib import import_module
    cli = import_module("squigly-trace_amd.cli")
    bih, _, _ = product_scene
    texts = [CAM_TEXTS[k] for k in ("camera", "moved", "rotated")]
    vf = tmp_path / "views"
    vf.write_bytes(b"\n".join(texts))
    monkeypatch.chdir(ROOT)
    out = str(tmp_path / "out" / "frame.png")
    assert cli.main(["-s", "3", "-d", "24,20", "--views", str(vf), "-p", out, "-c", str(tmp_path / "no-such-camera")]) == 0
    for i, t in enumerate(texts):
        got = tmp_path / "out" / f"frame_{i:04d}.png"
        ref = tmp_path / f"ref_{i}.png"
        sqt.write_png(str(ref), sqt.render_rgb8(bih, sqt.camera_from_text(t), 3, (24, 20)))
        assert got.read_bytes() == ref.read_bytes(), i
    assert not (tmp_path / "out" / "frame_0003.png").exists()
