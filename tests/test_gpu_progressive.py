"""Progressive rendering (sq_render_rows_device_range, DeviceScene.render_rows_range, Progressive, render_progressive and
the CLI's --preview-every): a frame rendered in sample ranges equals the frame of one call bit for bit, in every kernel form
and schedule, and every intermediate fold equals the oracle's left fold of its samples (src/Lib.hs:85-88)."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

import render_options as RO
from bitcmp import canon, ibits
from conftest import ROOT
from render_options import OPTION_TUPLES, THREADS
from scenes import emitter_soup_scene as soup, overflow_room

pytestmark = pytest.mark.gpu
set_options = functools.partial(RO.set_options, table=RO.FRAME)


@pytest.fixture(scope="module")
def dev(sqt, product_scene):
    assert sqt.device_count() >= 1, "no HIP device: the product has no CPU fallback"
    bih, _, _ = product_scene
    ds = sqt.DeviceScene(bih, 0)
    yield ds
    ds.close()


def one_call(ds, cam, n, w, h, cast=False, shard=(None, 0, 1)):
    """(avg, rgb) of render_rows and (avg, rgb, sums) of one range call [0, n), synchronised, on the host."""
    import torch
    a, r = ds.render_rows(cam, n, w, h, cast=cast, shard=shard)
    sums = torch.empty_like(a)
    ra, rr = ds.render_rows_range(cam, n, w, h, 0, n, sums, cast=cast, shard=shard)
    torch.cuda.synchronize()
    return (a.cpu(), r.cpu()), (ra.cpu(), rr.cpu(), sums.cpu())


def stepped(sqt, ds, cam, n, w, h, bounds, cast=False, shard=(None, 0, 1)):
    """The frame rendered in the ranges bounds[0:2], bounds[1:3], ... through Progressive: (avg, rgb, sums) on the host."""
    import torch
    assert bounds[0] == 0 and bounds[-1] == n
    p = sqt.Progressive(ds, cam, n, w, h, cast=cast, shard=shard)
    for a, b in zip(bounds, bounds[1:]):
        assert p.done == a
        avg, rgb = p.step(b - a)
    assert p.done == n and p.finished
    torch.cuda.synchronize()
    return avg.cpu(), rgb.cpu(), p.sums.cpu()


def assert_same(x, y, what):
    assert np.array_equal(ibits(x[0]), ibits(y[0])), (what, "avg")
    assert np.array_equal(x[1].numpy(), y[1].numpy()), (what, "rgb")
    if len(x) > 2 and len(y) > 2:
        assert np.array_equal(ibits(x[2]), ibits(y[2])), (what, "sums")


# ---- 1. split equals one call ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("small_slots", [False, True])
@pytest.mark.parametrize("opts", OPTION_TUPLES + ("pool0", "cast"))
def test_split_equals_one_call(sqt, product_scene, dev, opts, small_slots):
    """[0, N) in one range call, in 1-sample steps and in uneven steps equals render_rows(samples=N): avg, RGB8 and sums.
    small_slots: two samples per batch in one call (one per track when overlapped), so the calls span several internal batches
    and the step boundaries 7 and 2 fall inside batches of the one-call schedule."""
    _, cam, _ = product_scene
    w, h, n = 40, 30, 9
    cast = opts == "cast"
    if opts == "pool0":
        kw = {"pool": 0}
    elif opts == "cast":
        kw = {}
    else:
        kw = dict(zip(("variant", "resident", "profile", "overlap", "primary_pooled"), opts))
    set_options(dev, slots=(w * h * 2) if small_slots else (512 << 20), **kw)
    try:
        (a, r), whole = one_call(dev, cam, n, w, h, cast=cast)
        assert_same((a, r), whole, "one range call")
        for bounds in ([0, 2, 7, 9], list(range(n + 1)), [0, 5, 6, 9]):
            assert_same(stepped(sqt, dev, cam, n, w, h, bounds, cast=cast), whole, (opts, bounds))
    finally:
        set_options(dev)


# ---- 2. sums and previews against the oracle -------------------------------------------------------------------------
def oracle_fold_check(sqt, O, ds, cam_p, ob, cam_o, w, h, n, cast=False, nan_ok=False, bounds=None):
    """After every step k: sums == float32 left fold of the oracle's samples [0, k), avg == 1/k * fold, rgb == tonemap(avg)."""
    import torch
    if cast:   # the cast colour of a pixel is the oracle's 1-sample cast frame (1 / 1 * c == c)
        c, _, _ = ob.render(cam_o, 1, w, h, cast=True, threads=THREADS)
        samples = [c] * n
    else:
        samples = [np.array([[ob.sample_radiance(cam_o, n, w, h, y, x, k) for x in range(h)] for y in range(w)], np.float32)
                   for k in range(n)]
    p = sqt.Progressive(ds, cam_p, n, w, h, cast=cast)
    fold = np.zeros((w, h, 3), np.float32)
    bounds = bounds or list(range(n + 1))
    for a, b in zip(bounds, bounds[1:]):
        avg, rgb = p.step(b - a)
        torch.cuda.synchronize()
        for k in range(a, b):
            fold = fold + samples[k]
        want_avg = np.float32(1) / np.float32(b) * fold
        cmp = canon if nan_ok else ibits
        assert np.array_equal(cmp(p.sums), cmp(fold)), ("sums", b)
        assert np.array_equal(cmp(avg), cmp(want_avg)), ("avg", b)
        want_rgb = np.array([[O.tonemap(tuple(float(v) for v in want_avg[y, x])) for x in range(h)] for y in range(w)], np.uint8)
        assert np.array_equal(rgb.cpu().numpy(), want_rgb), ("rgb", b)
    return fold


def test_sums_and_previews_follow_the_oracle_fold(sqt, O, product_scene, oracle_scene, dev):
    _, cam, _ = product_scene
    ob, ocam, _ = oracle_scene
    set_options(dev)
    fold = oracle_fold_check(sqt, O, dev, cam, ob, ocam, 24, 20, 6)
    o, _, _ = ob.render(ocam, 6, 24, 20, threads=THREADS)         # the oracle's own render agrees with the fold
    assert np.array_equal(ibits(np.float32(1) / np.float32(6) * fold), ibits(o))
    oracle_fold_check(sqt, O, dev, cam, ob, ocam, 24, 20, 6, bounds=[0, 4, 6])
    set_options(dev, variant=1)
    try:
        oracle_fold_check(sqt, O, dev, cam, ob, ocam, 24, 20, 6, bounds=[0, 1, 5, 6])
    finally:
        set_options(dev)


def test_cast_sums_fold_the_oracle_cast_colour(sqt, O, product_scene, oracle_scene, dev):
    _, cam, _ = product_scene
    ob, ocam, _ = oracle_scene
    set_options(dev)
    oracle_fold_check(sqt, O, dev, cam, ob, ocam, 24, 20, 5, cast=True, bounds=[0, 2, 3, 5])


@pytest.mark.parametrize("which", ["soup", "overflow"])
def test_sums_follow_the_oracle_on_mirrors_emitters_and_overflow(sqt, O, which):
    bih, ob, cam_p, cam_o = soup(sqt, O, 4, 12) if which == "soup" else overflow_room(sqt, O)
    ds = sqt.DeviceScene(bih, 0)
    try:
        fold = oracle_fold_check(sqt, O, ds, cam_p, ob, cam_o, 24, 20, 6, nan_ok=True, bounds=[0, 1, 4, 6])
        if which == "overflow":
            assert np.isnan(fold).any()
        else:
            assert (fold > 0).any()
        ds.set_option("overlap", 2)
        oracle_fold_check(sqt, O, ds, cam_p, ob, cam_o, 24, 20, 6, nan_ok=True, bounds=[0, 3, 6])
    finally:
        ds.close()


# ---- 3. shards -------------------------------------------------------------------------------------------------------
def test_progressive_shards_are_rows_of_the_progressive_frame(sqt, product_scene, dev):
    from importlib import import_module
    d = import_module("squigly-trace_amd.dist")
    _, cam, _ = product_scene
    set_options(dev)
    w, h, n, bounds = 37, 24, 7, [0, 3, 4, 7]
    full = stepped(sqt, dev, cam, n, w, h, bounds)
    for r in range(3):
        part = stepped(sqt, dev, cam, n, w, h, bounds, shard=(2, r, 3))
        rows = d.shard_rows(w, 2, r, 3)
        assert part[0].shape[0] == len(rows) > 0
        assert_same(part, tuple(t[rows] for t in full), ("shard", r))


# ---- 4. 32-bit stack words, streaming forms --------------------------------------------------------------------------
def test_split_equals_one_call_with_32_bit_stack_words(sqt):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_scenes as G
    obj, sq, camt = G.heightfield_scene(130)
    bih = sqt.BIH(sqt.Mesh.from_text(obj, sq))
    assert bih.scene.n_tris > 0x8000
    cam = sqt.camera_from_text(camt)
    ds = sqt.DeviceScene(bih, 0)
    try:
        w, h, n = 32, 24, 5
        for variant in (2, 1):
            ds.set_option("variant", variant)
            (a, r), whole = one_call(ds, cam, n, w, h)
            assert_same((a, r), whole, "one range call")
            plan = ds.last_plan()
            assert plan["stack_word_bytes"] == 4
            print(f"[progressive] {bih.scene.n_tris} triangles, variant {variant}: trace_form {plan['trace_form']}")
            if variant == 2:
                assert plan["trace_form"] in ("streaming_six_wave", "streaming_plain")
            for bounds in ([0, 1, 3, 5], [0, 4, 5]):
                assert_same(stepped(sqt, ds, cam, n, w, h, bounds), whole, (variant, bounds))
    finally:
        ds.close()


# ---- 5. resume after a checkpoint ------------------------------------------------------------------------------------
def test_resume_from_a_host_checkpoint_in_a_new_scene(sqt, product_scene):
    import torch
    bih, cam, _ = product_scene
    w, h, n, k = 40, 30, 9, 4
    ds = sqt.DeviceScene(bih, 0)
    p = sqt.Progressive(ds, cam, n, w, h)
    p.step(3)
    p.step(1)
    torch.cuda.synchronize()
    saved_sums, saved_done = p.sums.cpu().numpy().copy(), p.done
    assert saved_done == k
    del p
    ds.close()
    ds = sqt.DeviceScene(bih, 0)
    try:
        q = sqt.Progressive(ds, cam, n, w, h, sums=torch.from_numpy(saved_sums).cuda(), done=saved_done)
        avg, rgb = q.step(n)
        assert q.done == n
        torch.cuda.synchronize()
        (a, r), whole = one_call(ds, cam, n, w, h)
        assert_same((avg.cpu(), rgb.cpu(), q.sums.cpu()), whole, "resumed")
        # a host array is adopted as well (copied to the device)
        q2 = sqt.Progressive(ds, cam, n, w, h, sums=saved_sums, done=saved_done)
        avg2, rgb2 = q2.step(n)
        torch.cuda.synchronize()
        assert_same((avg2.cpu(), rgb2.cpu(), q2.sums.cpu()), whole, "resumed from numpy")
    finally:
        ds.close()


# ---- 6. fresh frames and misses --------------------------------------------------------------------------------------
def test_fresh_frame_ignores_the_sums_and_misses_get_positive_zero(sqt, O):
    import torch
    bih, ob, cam_p, cam_o = soup(sqt, O, 4, 12)
    w, h, n = 24, 20, 4
    miss = np.array([[not ob.intersect(*O.make_ray(w, h, y, x, cam_o)).hit for x in range(h)] for y in range(w)])
    assert miss.any() and not miss.all()
    ds = sqt.DeviceScene(bih, 0)
    try:
        for opts in ({"variant": 1}, {}, {"resident": 0}, {"primary_resident": 0}, {"primary_pooled": 1}, {"overlap": 2}):
            ds.set_option("variant", 2); ds.set_option("resident", 1); ds.set_option("primary_resident", 1)
            ds.set_option("primary_pooled", 0); ds.set_option("overlap", 0)
            for k, v in opts.items():
                ds.set_option(k, v)
            (a, r), whole = one_call(ds, cam_p, n, w, h)
            for bounds in ([0, n], [0, 1, 3, n]):
                nan_sums = torch.full((w, h, 3), float("nan"), dtype=torch.float32, device="cuda:0")
                p = sqt.Progressive(ds, cam_p, n, w, h, sums=nan_sums)
                assert p.sums is nan_sums                             # a matching CUDA tensor is adopted, not copied
                for x, y in zip(bounds, bounds[1:]):
                    avg, rgb = p.step(y - x)
                torch.cuda.synchronize()
                got = (avg.cpu(), rgb.cpu(), p.sums.cpu())
                assert_same(got, whole, (opts, bounds))
                assert (ibits(got[2])[miss] == 0).all(), opts      # +0 bits, not -0 or NaN
    finally:
        ds.close()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------
def test_refusals_leave_every_buffer_untouched(sqt, product_scene, dev):
    import torch
    import tree_padding as TP
    bih, cam, _ = product_scene
    set_options(dev)
    w, h, n = 16, 12, 4
    L = sqt.lib()
    sh = sqt.Shard(w, 0, 1)
    dv = "cuda:0"
    sums = torch.full((w, h, 3), 7.25, dtype=torch.float32, device=dv)
    avg = torch.full((w, h, 3), -3.5, dtype=torch.float32, device=dv)
    rgb = torch.full((w, h, 3), 123, dtype=torch.uint8, device=dv)
    keep = (sums.clone(), avg.clone(), rgb.clone())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(ds_h, kb, ke, s_ptr, a_ptr, shard=sh, samples=n):
        return L.sq_render_rows_device_range(ds_h, C.byref(cam), samples, w, h, 0, shard, kb, ke, s_ptr, a_ptr, rgb.data_ptr(), stream)

    cases = {
        "k_begin < 0": (-1, 2, sums.data_ptr(), avg.data_ptr()),
        "k_end == k_begin": (2, 2, sums.data_ptr(), avg.data_ptr()),
        "k_end < k_begin": (3, 1, sums.data_ptr(), avg.data_ptr()),
        "k_end > samples": (0, n + 1, sums.data_ptr(), avg.data_ptr()),
        "d_sum NULL": (0, n, None, avg.data_ptr()),
        "d_sum == d_avg": (0, n, sums.data_ptr(), sums.data_ptr()),
    }
    for what, (kb, ke, s_ptr, a_ptr) in cases.items():
        assert call(dev._h, kb, ke, s_ptr, a_ptr) != 0, what
        assert len(L.sq_last_error()) > 0, what
    assert call(dev._h, 0, n, sums.data_ptr(), avg.data_ptr(), shard=sqt.Shard(2, 3, 3)) != 0        # bad shard
    assert b"bad shard" in L.sq_last_error()
    # LDS-height limits: 200 frames fit the per-pixel kernel's 256 lanes but not the streaming form's 512 (refused after the
    # workspace is planned); 400 fit no form
    for height, variant in ((200, 2), (400, 1), (400, 2)):
        ds = sqt.DeviceScene(TP.full_stack(bih, height, 0, TP.LEFT), 0)
        try:
            ds.set_option("variant", variant)
            assert call(ds._h, 1, n, sums.data_ptr(), avg.data_ptr()) != 0
            assert f"BIH height {height} needs".encode() in L.sq_last_error(), L.sq_last_error()
            assert ds.last_plan()["launched"] == 0
            torch.cuda.synchronize()
        finally:
            ds.close()
    with pytest.raises(sqt.SquiglyError):
        dev.render_rows_range(cam, n, w, h, 0, n, None)
    torch.cuda.synchronize()
    for got, want in zip((sums, avg, rgb), keep):
        assert torch.equal(got, want)


# ---- 8. CLI previews -------------------------------------------------------------------------------------------------
def test_cli_previews_end_in_the_same_file(sqt, tmp_path, monkeypatch, capsys):
    from importlib import import_module
    cli = import_module("squigly-trace_amd.cli")
    monkeypatch.chdir(ROOT)                                          # the reference's default obj and camera paths are relative
    plain, prev = str(tmp_path / "plain.png"), str(tmp_path / "preview.png")
    assert cli.main(["-s", "8", "-d", "64,64", "-p", plain]) == 0
    out = capsys.readouterr().out
    assert "Preview" not in out
    assert cli.main(["-s", "8", "-d", "64,64", "--preview-every", "3", "-p", prev]) == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Preview")]
    assert len(lines) == 3 and [ln.split()[1] for ln in lines] == ["3/8", "6/8", "8/8"], lines
    with open(plain, "rb") as f1, open(prev, "rb") as f2:
        assert f1.read() == f2.read()


def test_render_progressive_ends_in_render_rgb8(sqt, product_scene):
    bih, cam, _ = product_scene
    seen = list(sqt.render_progressive(bih, cam, 5, (20, 16), 2))
    assert [d for d, _ in seen] == [2, 4, 5]
    assert seen[-1][1].shape == (20, 16, 3) and seen[-1][1].dtype == np.uint8
    assert np.array_equal(seen[-1][1], sqt.render_rgb8(bih, cam, 5, (20, 16)))


# ---- 9. Progressive lifecycle ----------------------------------------------------------------------------------------
def test_progressive_step_clamps_then_raises(sqt, product_scene, dev):
    import torch
    _, cam, _ = product_scene
    set_options(dev)
    w, h, n = 12, 10, 5
    p = sqt.Progressive(dev, cam, n, w, h)
    assert (p.done, p.finished) == (0, False)
    assert tuple(p.sums.shape) == (w, h, 3) and p.sums.dtype == torch.float32
    p.step(3)
    assert p.done == 3
    avg, rgb = p.step(100)
    assert p.done == n and p.finished
    with pytest.raises(RuntimeError):
        p.step(1)
    with pytest.raises(ValueError):
        sqt.Progressive(dev, cam, n, w, h, done=2)                   # resuming needs the sums
    with pytest.raises(ValueError):
        sqt.Progressive(dev, cam, n, w, h, sums=p.sums, done=n + 1)
    with pytest.raises(ValueError):
        sqt.Progressive(dev, cam, n, w, h).step(0)
    torch.cuda.synchronize()
    (a, r), _ = one_call(dev, cam, n, w, h)
    assert np.array_equal(ibits(avg), ibits(a)) and torch.equal(rgb.cpu(), r)
