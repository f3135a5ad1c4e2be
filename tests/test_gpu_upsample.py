"""Sparse frames on the GPU: sq_denoise_sparse_mask_device and sq_denoise_upsample_device bit for bit (NaN = NaN) against the numpy
restatement (tests/upsample_restatement.py) at the shapes where indexing can go wrong, for every stride class and offset; and the
drivers on top (DeviceScene.render_rows_masked under the mask, sqt.Temporal(sparse=), render_sequence, render_sparse, the CLI) on the
project's own scene."""
import collections
import importlib
import os

import numpy as np
import pytest

import temporal_restatement as TRS
import temporal_room as TR
import upsample_restatement as R
from bitcmp import same, same_exact
from conftest import DATA, ROOT

pytestmark = pytest.mark.gpu
f32 = np.float32
G = collections.namedtuple("G", ["tri", "normal", "point"])
STRIDES = (1, 2, 3, 4, 8, 16)
STOPS = dict(sigma_p=0.05, cos_n=0.9)
_CACHE = {}


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def dn(sqt, torch):
    mod = importlib.import_module("squigly-trace_amd.denoise")
    mod.lib()
    return mod


def offsets(s):
    """Every offset for s <= 3, the four corner offsets above that."""
    return [(oy, ox) for oy in range(s) for ox in range(s)] if s <= 3 else [(oy, ox) for oy in (0, s - 1) for ox in (0, s - 1)]


def frame(rows, cols, seed=7):
    key = (rows, cols, seed)
    if key not in _CACHE:
        _CACHE[key] = R.synthetic(rows, cols, seed)
    return _CACHE[key]


def dev(torch, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def gpu_frame(torch, fr):
    color, var, tri, nrm, pnt = (dev(torch, a) for a in fr)
    return color, var, G(tri, nrm, pnt)


def check_lattice(torch, dn, fr, dfr, s, off, with_var, stops=STOPS, label=None):
    """Both calls for one lattice against the restatement; returns the restated mask."""
    color, var, tri, nrm, pnt = fr
    d_color, d_var, g = dfr
    label = label or (tri.shape, s, off, with_var)
    want_mask = R.sparse_mask(tri, nrm, pnt, s, *off, **stops)
    mask = dn.sparse_mask(g, s, off, **stops)
    assert mask.dtype == torch.uint8 and np.array_equal(mask.cpu().numpy(), want_mask), (label, "mask")
    want, want_var = R.upsample(color, tri, nrm, pnt, want_mask, s, *off, var=var if with_var else None, **stops)
    out, out_var = dn.upsample(d_color, g, mask, s, off, var=d_var if with_var else None, **stops)
    assert same(out.cpu().numpy(), want), (label, "colour")
    assert (out_var is None and want_var is None) if not with_var else same(out_var.cpu().numpy(), want_var), (label, "variance")
    return want_mask


SIZES = [(1, 1), (1, 9), (9, 1), (2, 2), (17, 33), (70, 131)]


@pytest.mark.parametrize("rows, cols", SIZES, ids=[f"{r}x{c}" for r, c in SIZES])
def test_both_calls_are_the_restatement(torch, dn, rows, cols):
    """Every stride of STRIDES, every offset (the corner offsets above stride 3), with and without variance.  17 x 33 and 70 x 131 are
    multiples of no stride, of 64 and of no tile, and 70 x 131 crosses workgroup edges both ways."""
    fr = frame(rows, cols)
    dfr = gpu_frame(torch, fr)
    seen = collections.Counter()
    for s in STRIDES:
        for off in offsets(s):
            for with_var in (True, False):
                m = check_lattice(torch, dn, fr, dfr, s, off, with_var)
            lat = R.lattice(rows, cols, s, *off)
            yy, xx = np.mgrid[0:rows, 0:cols]
            seen.update(holes=int(((m != 0) & ~lat).sum()), filled_hit=int(((m == 0) & (fr[2] >= 0)).sum()),
                        filled_sky=int(((m == 0) & (fr[2] < 0)).sum()), before=int(((m == 0) & ((yy < off[0]) | (xx < off[1]))).sum()))
    if rows >= 17:                # misses, back-facing and far taps make holes; hit and sky pixels are filled in, before the lattice too
        assert all(seen[k] > 0 for k in ("holes", "filled_hit", "filled_sky", "before")), seen


@pytest.mark.parametrize("s", STRIDES)
def test_one_cell_and_a_pixel(torch, dn, s):
    """(s + 1) x (s + 1): one whole cell of the lattice at offset (0, 0), and one row and column short of it at the other corners."""
    fr = frame(s + 1, s + 1, seed=11)
    dfr = gpu_frame(torch, fr)
    for off in offsets(s):
        for with_var in (True, False):
            check_lattice(torch, dn, fr, dfr, s, off, with_var)


def test_stride_one_is_the_identity(torch, dn):
    fr = R.synthetic(17, 33, seed=3, odd=True)
    color, var, g = gpu_frame(torch, fr)
    mask = dn.sparse_mask(g, 1, (0, 0), **STOPS)
    assert bool(mask.all())
    out, out_var = dn.upsample(color, g, mask, 1, (0, 0), var=var, **STOPS)
    assert same_exact(out, color) and same_exact(out_var, var)                 # the inputs' own bits, NaN payloads too


def test_what_was_not_traced_is_never_read(torch, dn):
    """The pixels the mask leaves out hold NaN, or anything else, on entry: the output is the same bits; and a traced pixel comes
    through with its own bits, NaN payloads included."""
    fr = frame(70, 131)
    color, var, tri, nrm, pnt = fr
    d_color, d_var, g = gpu_frame(torch, fr)
    for s, off in ((2, (1, 0)), (3, (2, 2)), (8, (7, 0))):
        mask = dn.sparse_mask(g, s, off, **STOPS)
        dead = mask == 0
        assert bool(dead.any())
        base = dn.upsample(d_color, g, mask, s, off, var=d_var, **STOPS)
        payload = torch.tensor([0x7FC12345], dtype=torch.int32, device="cuda").view(torch.float32)
        for poison in (float("nan"), -1e30):
            pc, pv = torch.where(dead[..., None], poison, d_color), torch.where(dead, poison, d_var)
            live = torch.nonzero(~dead)[:3]
            for y, x in live.tolist():                                      # traced pixels with a NaN of a payload of their own
                pc[y, x, 1], pv[y, x] = payload[0], payload[0]
            got = dn.upsample(pc, g, mask, s, off, var=pv, **STOPS)
            assert same_exact(got[0][~dead], pc[~dead]) and same_exact(got[1][~dead], pv[~dead])
            keep = torch.ones_like(dead)
            for y, x in live.tolist():                                      # (what the payload pixels are taps of differs, as it must)
                keep[max(0, y - s):y + s + 1, max(0, x - s):x + s + 1] = False
            assert same_exact(got[0][keep], base[0][keep]) and same_exact(got[1][keep], base[1][keep])
            assert not bool(torch.isnan(got[0][dead & keep]).any())


def test_a_callers_masks(torch, dn):
    """An all-zero mask: the lattice is still copied through and the holes take the second copy-through branch; an all-one mask: the
    identity.  Both against the restatement."""
    fr = frame(17, 33)
    color, var, tri, nrm, pnt = fr
    d_color, d_var, g = gpu_frame(torch, fr)
    for s, off in ((2, (0, 1)), (4, (3, 3))):
        own = R.sparse_mask(tri, nrm, pnt, s, *off, **STOPS)
        holes = (own != 0) & ~R.lattice(17, 33, s, *off)
        assert holes.any()
        zeros = np.zeros((17, 33), np.uint8)
        want, want_var = R.upsample(color, tri, nrm, pnt, zeros, s, *off, var=var, **STOPS)
        got, got_var = dn.upsample(d_color, g, dev(torch, zeros), s, off, var=d_var, **STOPS)
        assert same(got.cpu().numpy(), want) and same(got_var.cpu().numpy(), want_var)
        assert same(want[holes], color[holes]) and not same(want, color)
        ones = dev(torch, np.ones((17, 33), np.uint8))
        got, got_var = dn.upsample(d_color, g, ones, s, off, var=d_var, **STOPS)
        assert same_exact(got, d_color) and same_exact(got_var, d_var)
        # outputs the caller gives are the ones that are filled
        out = (torch.full_like(d_color, -7.0), torch.full_like(d_var, -7.0))
        res = dn.upsample(d_color, g, ones, s, off, var=d_var, out=out, **STOPS)
        assert res[0] is out[0] and res[1] is out[1] and same_exact(out[0], d_color) and same_exact(out[1], d_var)


def test_stops_at_equality_and_special_values(torch, dn):
    """Exact planes (n_p . n_q = 1, pd = 0 or 1): both stops accept equality and refuse one ulp past it; and guides and images with
    NaN, +-inf and -0 in every field."""
    rows, cols = 9, 14
    yy, xx = np.mgrid[0:rows, 0:cols]
    tri = np.zeros((rows, cols), np.int32)
    nrm = np.tile(np.array([0, 0, 1], f32), (rows, cols, 1))
    pnt = np.stack([xx, yy, (xx >= 7)], -1).astype(f32)
    rng = np.random.default_rng(5)
    fr = (rng.random((rows, cols, 3)).astype(f32), rng.random((rows, cols)).astype(f32), tri, nrm, pnt)
    dfr = gpu_frame(torch, fr)
    up = float(np.nextafter(f32(1), f32(2)))
    down = float(np.nextafter(f32(1), f32(0)))
    holes = []
    for stops in (dict(sigma_p=1.0, cos_n=1.0), dict(sigma_p=down, cos_n=1.0), dict(sigma_p=0.0, cos_n=1.0), dict(sigma_p=1.0, cos_n=up)):
        m = check_lattice(torch, dn, fr, dfr, 4, (0, 1), True, stops=stops)
        holes.append(int(((m != 0) & ~R.lattice(rows, cols, 4, 0, 1)).sum()))
    assert holes[0] == 0 and holes[1] == 0 and holes[2] == 0 and holes[3] == (~R.lattice(rows, cols, 4, 0, 1)).sum()
    w1 = R.upsample(fr[0], tri, nrm, pnt, np.zeros((rows, cols), np.uint8), 4, 0, 1, sigma_p=1.0, cos_n=1.0)[0]
    w2 = R.upsample(fr[0], tri, nrm, pnt, np.zeros((rows, cols), np.uint8), 4, 0, 1, sigma_p=down, cos_n=1.0)[0]
    assert not same(w1, w2)                                                  # the taps across the step are taken at equality only
    odd = R.synthetic(17, 33, seed=9, odd=True)
    dodd = gpu_frame(torch, odd)
    for s, off in ((2, (0, 0)), (3, (1, 2)), (16, (15, 0))):
        check_lattice(torch, dn, odd, dodd, s, off, True)
    hand = R.handmade()
    dhand = gpu_frame(torch, hand)
    for s in (1, 2, 3):
        for off in offsets(s):
            check_lattice(torch, dn, hand, dhand, s, off, True, stops=dict(sigma_p=0.5, cos_n=0.5))


def test_more_tiles_than_blocks(torch, dn):
    """262152 x 3: 65538 tiles of 4 rows x 64 columns against the 65536 blocks of a launch, so both kernels' tile loops run more than
    once -- the small shapes never take that path."""
    rows, cols = 4 * 65536 + 8, 3
    fr = tuple(np.concatenate([a] * 24) for a in R.synthetic(rows // 24, cols, seed=13))       # (a seeded strip, 24 times over)
    assert fr[2].shape == (rows, cols)
    dfr = gpu_frame(torch, fr)
    m = check_lattice(torch, dn, fr, dfr, 2, (1, 1), True)
    assert (m[-8:] == 0).any() and (m[:8] == 0).any()


def test_python_layer_refusals(torch, dn):
    fr = frame(5, 7, seed=1)
    color, var, g = gpu_frame(torch, fr)
    mask = dn.sparse_mask(g, 2, (0, 0), **STOPS)
    E = dn.N.SquiglyError
    with pytest.raises(E, match="guides.tri must be"):
        dn.sparse_mask(G(g.tri.float(), g.normal, g.point), 2, (0, 0), **STOPS)
    with pytest.raises(E, match="guides.normal must be"):
        dn.sparse_mask(G(g.tri, g.normal[:, :6], g.point), 2, (0, 0), **STOPS)
    with pytest.raises(E, match="mask must be"):
        dn.upsample(color, g, mask.int(), 2, (0, 0), **STOPS)
    with pytest.raises(E, match="var must be"):
        dn.upsample(color, g, mask, 2, (0, 0), var=var[:, :6], **STOPS)
    with pytest.raises(E, match="an output variance needs var"):
        dn.upsample(color, g, mask, 2, (0, 0), out=(torch.empty_like(color), torch.empty_like(var)), **STOPS)
    with pytest.raises(E, match="d_color and d_out overlap"):
        dn.upsample(color, g, mask, 2, (0, 0), out=color, **STOPS)
    with pytest.raises(E, match="sigma_p must be"):
        dn.sparse_mask(g, 2, (0, 0), sigma_p=-1.0)
    with pytest.raises(E, match="cos_n must be"):
        dn.upsample(color, g, mask, 2, (0, 0), sigma_p=0.05, cos_n=float("nan"))


# ---- the room: real guides, the renderer's own samples ----
@pytest.fixture(scope="module")
def scene(sqt, torch, product_scene):
    bih, _, _ = product_scene
    ds = sqt.DeviceScene(bih, 0)
    yield ds
    torch.cuda.synchronize()
    ds.close()


def host_guides(g):
    return g.tri.cpu().numpy(), g.normal.cpu().numpy(), g.point.cpu().numpy()


def dense_moments(torch, ds, cam, samples, k0, k1):
    w, h = TR.W, TR.H
    sums = torch.zeros((w, h, 3), dtype=torch.float32, device="cuda")
    sums2 = torch.zeros_like(sums)
    ds.render_rows_masked(cam, samples, w, h, k0, k1, sums, sums2=sums2, want_avg=False, want_rgb=False)
    return sums, sums2


@pytest.mark.parametrize("s, off", [(2, (0, 0)), (2, (1, 1)), (4, (0, 0))], ids=["s2-00", "s2-11", "s4-00"])
def test_a_traced_pixel_is_the_dense_frames(sqt, torch, dn, scene, s, off):
    """The room under camera 0 of the sequence: the mask of the device's own guides is the restatement's and has both kinds of live
    pixel; the masked call under it leaves the dense frame's bits at every live pixel and writes no other; and the frame filled in is
    the restatement's."""
    w, h, spp = TR.W, TR.H, 4
    cam = sqt.camera_from_text(TR.CAMERA_TEXTS[0])
    sp = dn.default_sigma_p(scene.bih.bounds)
    g = scene.guides(cam, w, h)
    mask = dn.sparse_mask(g, s, off, sigma_p=sp)
    tri, nrm, pnt = host_guides(g)
    want_mask = R.sparse_mask(tri, nrm, pnt, s, *off, sigma_p=sp, cos_n=0.9)
    assert np.array_equal(mask.cpu().numpy(), want_mask)
    lat = R.lattice(w, h, s, *off)
    holes, filled_hits = int(((want_mask != 0) & ~lat).sum()), int(((want_mask == 0) & (tri >= 0)).sum())
    assert 10 <= holes <= 0.05 * w * h and filled_hits >= 900, (holes, filled_hits)
    dense, dense2 = dense_moments(torch, scene, cam, spp, 0, spp)
    sums = torch.zeros_like(dense)
    sums2 = torch.zeros_like(dense)
    avg, _ = scene.render_rows_masked(cam, spp, w, h, 0, spp, sums, mask=mask, sums2=sums2, want_rgb=False)
    dense_avg, _ = scene.render_rows_range(cam, spp, w, h, 0, spp, torch.zeros_like(dense), want_rgb=False)
    live = mask != 0
    assert same_exact(sums[live], dense[live]) and same_exact(sums2[live], dense2[live]) and same_exact(avg[live], dense_avg[live])
    assert not bool(sums[~live].any()) and not bool(sums2[~live].any()) and not bool(avg[~live].any())
    assert bool((dense[~live] != 0).any())
    var = dn.denoise_variance(sums, sums2, torch.full((w, h), spp, dtype=torch.int32, device="cuda"))
    out, out_var = dn.upsample(avg, g, mask, s, off, var=var, sigma_p=sp)
    want, want_var = R.upsample(avg.cpu().numpy(), tri, nrm, pnt, want_mask, s, *off, var=var.cpu().numpy(), sigma_p=sp, cos_n=0.9)
    assert same(out.cpu().numpy(), want) and same(out_var.cpu().numpy(), want_var)
    assert bool((out[~live] != 0).any())


def restated_step(torch, dn, tp, ds, cam, f, spp, period, sparse, params, prev_cam, prev):
    """A Temporal(sparse=).step restated: the dense frame's moments from the renderer and the demodulation by the package's own torch
    helpers -- neither is new -- and between them the mask and the fill, then the accumulation, in numpy.  The pixels the mask leaves
    out are overwritten with NaN before the fill: the step may not have read them."""
    w, h = TR.W, TR.H
    k0 = (f % period) * spp
    sums, sums2 = dense_moments(torch, ds, cam, spp * period, k0, k0 + spp)
    noisy = sums / float(spp)
    var = dn.denoise_variance(sums, sums2, torch.full((w, h), spp, dtype=torch.int32, device="cuda"))
    g = ds.guides(cam, w, h)
    x, v, how = dn.demodulated(g, noisy, var)
    tri, nrm, pnt = host_guides(g)
    off = R.lattice_offset(f, sparse)
    mask, xs, vs = R.sparse_frame(x.cpu().numpy(), v.cpu().numpy(), tri, nrm, pnt, sparse, *off, sigma_p=params["sigma_p"], cos_n=params["cos_n"])
    acc = TRS.accumulate(xs, vs, tri, nrm, pnt, prev_cam, prev, alpha=tp.frame_alpha(ds, g.tri).cpu().numpy(), **params)
    out, out_var = dn.remodulated(g, dev(torch, acc["color"]), dev(torch, acc["var"]), how)
    return dict(out=out, out_var=out_var, len=acc["len"], block=acc["block"], mask=mask, noisy=noisy)


def test_three_sparse_steps_and_a_resume(sqt, torch, dn, scene):
    """Three steps of sqt.Temporal(sparse=2) under the moving cameras against the restated chain, with a checkpoint after the second:
    the resumed sequence and the one that went on both give the chain's third frame."""
    tp = importlib.import_module("squigly-trace_amd.temporal")
    spp, period = 4, 8
    cams = [sqt.camera_from_text(t) for t in TR.CAMERA_TEXTS[:3]]
    t = sqt.Temporal(scene, TR.W, TR.H, spp, period=period, sparse=2)
    assert t.sparse == 2 and t.live is None
    params = dict(t.params)
    prev, prev_cam, saved, offsets_seen = None, None, None, []
    for f, cam in enumerate(cams):
        want = restated_step(torch, dn, tp, scene, cam, f, spp, period, 2, params, prev_cam, prev)
        runs = [t]
        if f == 2:
            runs.append(sqt.Temporal(scene, TR.W, TR.H, spp, period=period, sparse=2, history=saved[0], camera=saved[1], frames=saved[2]))
        for run in runs:
            avg, var, length, rgb = run.step(cam)
            torch.cuda.synchronize()
            live = want["mask"] != 0
            assert np.array_equal(run.live.cpu().numpy(), want["mask"]), f
            assert same(avg.cpu().numpy(), want["out"].cpu().numpy()) and same(var.cpu().numpy(), want["out_var"].cpu().numpy()), f
            assert np.array_equal(length.cpu().numpy(), want["len"]), f
            assert same_exact(run.noisy[dev(torch, live)], want["noisy"][dev(torch, live)])       # meaningful on the live pixels only
            assert not bool(run.noisy[dev(torch, ~live)].any())
            got = tp.unpack(run.history, TR.W, TR.H)
            for name in TRS.BLOCK_FIELDS:
                a, b = getattr(got, name).cpu().numpy(), want["block"][name]
                assert (same(a, b) if b.dtype == f32 else np.array_equal(a, b)), (f, name)
            assert rgb.dtype == torch.uint8 and bool((rgb > 0).any())
        offsets_seen.append(R.lattice_offset(f, 2))
        assert 0.2 < want["mask"].mean() < 0.35
        if f == 1:
            saved = (t.history.cpu().numpy().copy(), sqt.Camera.from_buffer_copy(bytes(t.camera)), t.frames)
        prev, prev_cam = want["block"], cam
    assert offsets_seen == [(0, 0), (1, 1), (0, 1)] and t.frames == 3
    assert (want["len"] == 3).any() and (want["len"] == 1).any()


def test_sparse_none_is_the_sequence_as_it_was(sqt, torch, scene):
    cams = [sqt.camera_from_text(t) for t in TR.CAMERA_TEXTS[:3]]
    a = sqt.Temporal(scene, TR.W, TR.H, 4, period=8, denoise={"passes": 2})
    b = sqt.Temporal(scene, TR.W, TR.H, 4, period=8, denoise={"passes": 2}, sparse=None)
    c = sqt.Temporal(scene, TR.W, TR.H, 4, period=8, denoise={"passes": 2}, sparse=2)
    assert a.sparse is None and b.sparse is None
    differs = False
    for cam in cams:
        ra, rb, rc = a.step(cam), b.step(cam), c.step(cam)
        torch.cuda.synchronize()
        assert same_exact(ra, rb) and same_exact(a.noisy, b.noisy) and same_exact(a.history, b.history)
        assert a.live is None and b.live is None and c.live is not None
        differs |= not same_exact(ra[:2], rc[:2])
    assert differs


def test_render_sequence_sparse_and_the_cli(sqt, torch, product_scene, tmp_path, monkeypatch):
    """render_sequence(sparse=2) and the CLI's --sequence --temporal --sparse 2 write the same PNG bytes, and both differ from the
    dense sequence; render_sparse at stride 1 without demodulation is render_rgb8, and at stride 2 it keeps the traced pixels."""
    bih, cam, _ = product_scene
    cams = [sqt.camera_from_text(t) for t in TR.CAMERA_TEXTS[:3]]
    dense = list(sqt.render_sequence(bih, cams, 4, (TR.W, TR.H)))
    sparse = list(sqt.render_sequence(bih, cams, 4, (TR.W, TR.H), sparse=2))
    assert len(sparse) == 3 and all(i.shape == (TR.W, TR.H, 3) and i.dtype == np.uint8 for i in sparse)
    assert all(not np.array_equal(a, b) for a, b in zip(dense, sparse))
    cli = importlib.import_module("squigly-trace_amd.cli")
    monkeypatch.chdir(ROOT)
    seq = tmp_path / "move.cams"
    seq.write_bytes(b"".join(TR.CAMERA_TEXTS[:3]))
    path = tmp_path / "move.png"
    assert cli.main(["-s", "4", "-d", f"{TR.W},{TR.H}", "-p", str(path), "--objpath", os.path.join(DATA, "scene.obj"),
                     "--sequence", str(seq), "--temporal", "--sparse", "2"]) == 0
    for i, p in enumerate(cli.view_paths(str(path), 3)):
        ours = tmp_path / f"ours_{i}.png"
        sqt.write_png(str(ours), sparse[i])
        assert open(p, "rb").read() == open(ours, "rb").read(), i
    full = sqt.render_rgb8(bih, cam, 4, (TR.W, TR.H))
    assert np.array_equal(sqt.render_sparse(bih, cam, 4, (TR.W, TR.H), 1, demodulate=False), full)
    half = sqt.render_sparse(bih, cam, 4, (TR.W, TR.H), 2, offset=(1, 0), demodulate=False)
    lat = R.lattice(TR.W, TR.H, 2, 1, 0)
    assert np.array_equal(half[lat], full[lat]) and not np.array_equal(half, full)
    filtered = sqt.render_sparse(bih, cam, 4, (TR.W, TR.H), 2, denoise=True)
    assert filtered.shape == full.shape and filtered.any() and not np.array_equal(filtered, half)
