"""Anti-aliasing and depth of field on the GPU (libsquigly_lens.so, DeviceScene.lens_rays / render_lens): the ray kernel, the fold
kernel and whole frames equal tests/lens_restatement.py (pinned to the oracle by tests/test_lens.py) bit for bit with NaN = NaN,
whole, in sub-ray ranges and in every batching; without jitter and aperture a frame is the main library's own; refusals leave every
buffer as it was.  (The call on a gated non-blocking stream is tests/test_gpu_streams_lens.py.)"""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import depth_restatement as DR
import lens_restatement as LR
import sky_restatement as SR
import tree_padding as TP
from bitcmp import bits, ibits, nan_eq, same_exact
from conftest import DATA, GOLDEN, ROOT
from masked_calls import buffers, host, masked
from render_options import set_sky_options as set_options

pytestmark = pytest.mark.gpu
f32 = np.float32
W, H, S = LR.W, LR.H, LR.S
P = W * H


class Room:
    pass


@pytest.fixture(scope="module")
def room(sqt):
    import torch
    r = Room()
    r.c, r.ocam = LR.room()
    r.cam = sqt.load_camera(os.path.join(DATA, "camera"))
    r.ds = sqt.DeviceScene(r.c.bih, 0)
    r.bright = DR.case("bright")                 # the same room under materials that let most samples carry light: the frames' scene
    r.bds = sqt.DeviceScene(r.bright.bih, 0)
    r.lens = importlib.import_module("squigly-trace_amd.lens")
    r.lens.lib()
    r.torch = torch
    yield r
    torch.cuda.synchronize()
    r.ds.close()
    r.bds.close()


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def assert_rays(got, want, label):
    (o, d, s), (wo, wd, ws) = got, want
    o, d, s = (t.cpu().numpy() for t in (o, d, s))
    nb = wo.shape[0]
    assert o.shape[0] == nb and o.reshape(nb, -1, 3).shape == wo.shape
    for name, g, e in (("origins", o, wo), ("directions", d, wd)):
        ok = nan_eq(g.reshape(e.shape), e).all(-1)
        assert ok.all(), (label, name, int((~ok).sum()), np.argwhere(~ok)[:4])
    assert np.array_equal(s.reshape(ws.shape), ws), (label, "seeds")


# ---- 1. the ray kernel -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 2, 4, 8])
@pytest.mark.parametrize("jitter", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("aperture", [0.0, 0.1])
def test_rays_equal_the_restatement(sqt, room, R, jitter, aperture):
    lens = (jitter, aperture, 3.0)
    got = room.ds.lens_rays(room.cam, sqt.Lens(*lens), S, R, W, H)
    assert_rays(got, LR.rays(room.ocam, lens, S, R, W, H), (R, lens))
    if jitter == 0 and aperture == 0:                       # makeRay's rays and the frame's seeds, from the main library itself
        co, cd = room.ds.camera_rays(room.cam, W, H)
        seeds = sqt.frame_seeds(S, W, H).cuda()
        for r in range(R):
            assert same_exact(got[0][r], co) and same_exact(got[1][r], cd)
            assert room.torch.equal(got[2][r], seeds + r * (S // R))


def test_rays_of_less_than_a_wave_and_of_a_range(sqt, room):
    lens = LR.LENSES["both"]
    got = room.ds.lens_rays(room.cam, sqt.Lens(*lens), 6, 3, 5, 7)
    assert got[0].shape == (3, 5, 7, 3) and got[2].shape == (3, 5, 7)
    want = LR.rays(room.ocam, lens, 6, 3, 5, 7)
    assert_rays(got, want, "5 x 7")
    part = room.ds.lens_rays(room.cam, sqt.Lens(*lens), 6, 3, 5, 7, r_range=(1, 3))
    assert_rays(part, tuple(a[1:3] for a in want), "5 x 7, sub-rays 1 and 2")


def test_rays_of_a_shard(sqt, room):
    lens, shard = LR.LENSES["both"], (2, 1, 3)
    rows = DR.shard_rows(40, shard)
    got = room.ds.lens_rays(room.cam, sqt.Lens(*lens), 6, 2, 40, 72, shard=shard)
    assert got[0].shape == (2, len(rows), 72, 3)
    assert_rays(got, LR.rays(room.ocam, lens, 6, 2, 40, 72, rows=rows), "40 x 72, shard 1 of 3")
    co, cd = room.ds.camera_rays(room.cam, 40, 72, shard)
    plain = room.ds.lens_rays(room.cam, sqt.Lens(0, 0, 1), 6, 2, 40, 72, shard=shard)
    assert same_exact(plain[0][1], co) and same_exact(plain[1][1], cd)
    assert room.torch.equal(plain[2][1], sqt.frame_seeds(6, 40, 72, shard).cuda() + 3)


# ---- 2. the fold kernel ----------------------------------------------------------------------------------------------
def fold_call(room, parts, S_, r0, sum_, sum2, want_avg=True, want_rgb=True):
    torch = room.torch
    nb, p = parts.shape[0], parts.shape[1]
    avg = torch.full((p, 3), -3.5, dtype=torch.float32, device="cuda:0") if want_avg else None
    rgb = torch.full((p, 3), 123, dtype=torch.uint8, device="cuda:0") if want_rgb else None
    rc = room.lens.lib().sq_lens_fold_device(0, p, S_, r0, r0 + nb, cuda(parts).data_ptr(), sum_.data_ptr(), None if sum2 is None else sum2.data_ptr(),
                                             None if avg is None else avg.data_ptr(), None if rgb is None else rgb.data_ptr(), None)
    room.lens.check(rc)
    torch.cuda.synchronize()
    return avg, rgb


@pytest.mark.parametrize("p", [35, 384])
@pytest.mark.parametrize("nb", [1, 3])
def test_fold_equals_a_numpy_left_fold(room, p, nb):
    torch = room.torch
    rng = np.random.default_rng([p, nb])
    parts = (rng.standard_normal((nb + 2, p, 3)) * 10.0 ** rng.integers(-3, 4, (nb + 2, p, 3))).astype(f32)
    for i, v in enumerate((-0.0, np.inf, -np.inf, np.nan, 0.0, 3e38)):          # every special value in every block, also alone in its pixel
        parts[:, i, :] = v
        parts[i % (nb + 2), 8 + i, i % 3] = v
    parts[0, 20] = -0.0                                                          # s_0 = -0 with finite sums after it
    S_ = 2 * (nb + 2)
    # from s_0
    sum_ = torch.full((p, 3), 7.25, dtype=torch.float32, device="cuda:0")        # what the buffers hold is ignored when r_begin == 0
    sum2 = torch.full((p, 3), 5.5, dtype=torch.float32, device="cuda:0")
    avg, rgb = fold_call(room, parts[:nb], S_, 0, sum_, sum2)
    ws, wq, wa = LR.fold(parts, S_, (0, nb))
    for name, g, e in (("sum", sum_, ws), ("sum2", sum2, wq), ("avg", avg, wa)):
        assert nan_eq(g, e).all(), (name, np.argwhere(~nan_eq(g, e))[:4])
    assert np.array_equal(rgb.cpu().numpy(), LR.tonemap(wa))
    if nb == 1:
        real = ~np.isnan(parts[0])
        assert np.array_equal(ibits(sum_)[real], ibits(parts[0])[real])                      # s_0 itself, -0 included
        assert np.signbit(sum_.cpu().numpy()[20]).all()
    # carried on from a previous range: two more blocks onto what the buffers hold
    avg2, rgb2 = fold_call(room, parts[nb:], S_, nb, sum_, sum2)
    ws2, wq2, wa2 = LR.fold(parts, S_, (nb, nb + 2), ws, wq)
    whole = LR.fold(parts, S_)
    assert nan_eq(ws2, whole[0]).all() and nan_eq(wq2, whole[1]).all()
    for name, g, e in (("sum", sum_, ws2), ("sum2", sum2, wq2), ("avg", avg2, wa2)):
        assert nan_eq(g, e).all(), ("carried", name, np.argwhere(~nan_eq(g, e))[:4])
    assert np.array_equal(rgb2.cpu().numpy(), LR.tonemap(wa2))
    # without the optional buffers
    only = torch.full((p, 3), 1.0, dtype=torch.float32, device="cuda:0")
    assert fold_call(room, parts, S_, 0, only, None, want_avg=False, want_rgb=False) == (None, None)
    assert nan_eq(only, whole[0]).all()


# ---- 3. whole frames ---------------------------------------------------------------------------------------------------
UNDER = {"depth3": (3, None), "depth5": (5, None), "sky": (3, SR.GRADIENT)}
OPTIONS = {"default": {}, "variant1": {"variant": 1}, "resident0": {"resident": 0}}
_WANT = {}


def want_frame(lens_name, R, under):
    key = (lens_name, R, under)
    if key not in _WANT:
        depth, sky = UNDER[under]
        parts = LR.sub_ray_sums(LR.room_trails(lens_name, R), depth, sky)
        s, q, avg = LR.fold(parts, S)
        _WANT[key] = (parts, s, q, avg, LR.tonemap(avg))
    return _WANT[key]


def assert_frame(got, want, label):
    _, s, q, avg, rgb = want
    for name, g, e in (("sum", got.sum, s), ("sum2", got.sum2, q), ("avg", got.avg, avg)):
        ok = nan_eq(g.cpu().numpy().reshape(-1, 3), e).all(-1)
        assert ok.all(), (label, name, int((~ok).sum()), np.nonzero(~ok)[0][:6])
    assert np.array_equal(got.rgb.cpu().numpy().reshape(-1, 3), rgb), (label, "rgb")


@pytest.mark.parametrize("under", list(UNDER))
@pytest.mark.parametrize("opts", list(OPTIONS))
def test_frames_equal_the_restatement(sqt, room, under, opts):
    ds, lens_mod = room.bds, room.lens
    depth, sky = UNDER[under]
    lens = sqt.Lens(*LR.LENSES["both"])
    want = want_frame("both", 8, under)
    assert (want[1] != 0).any(-1).sum() > 100 and len(np.unique(ibits(want[0]).reshape(8, -1), axis=0)) == 8       # the sub-rays differ
    try:
        set_options(ds, sky=sky, depth=depth, **OPTIONS[opts])
        # whole
        whole = ds.render_lens(room.cam, lens, S, 8, W, H, want_sum2=True)
        assert_frame(whole, want, (under, opts, "whole"))
        # in sub-ray ranges
        first = ds.render_lens(room.cam, lens, S, 8, W, H, r_range=(0, 3), want_sum2=True)
        ps, pq, pavg = LR.fold(want[0], S, (0, 3))
        assert nan_eq(first.sum.cpu().numpy().reshape(-1, 3), ps).all() and nan_eq(first.avg.cpu().numpy().reshape(-1, 3), pavg).all()
        rest = ds.render_lens(room.cam, lens, S, 8, W, H, r_range=(3, 8), sums=(first.sum, first.sum2))
        assert rest.sum is first.sum and rest.sum2 is first.sum2
        assert_frame(rest, want, (under, opts, "ranges"))
        # a workspace that forces batches of 3, 3, 2
        nbytes = lens_mod.work_bytes(P, 3)
        assert lens_mod.plan(P, 0, 8, nbytes) == [(0, 3), (3, 6), (6, 8)]
        batched = ds.render_lens(room.cam, lens, S, 8, W, H, want_sum2=True, work_mb=nbytes / 2 ** 20)
        assert_frame(batched, want, (under, opts, "batches"))
        assert same_exact(tuple(batched), tuple(whole))
        # n = 2 samples on each of four sub-rays
        four = ds.render_lens(room.cam, lens, S, 4, W, H, want_sum2=True)
        assert_frame(four, want_frame("both", 4, under), (under, opts, "R = 4"))
    finally:
        set_options(ds)


# ---- 4. the pins on the device -------------------------------------------------------------------------------------------
def test_one_plain_sub_ray_is_the_committed_golden_frame(sqt, room):
    g_avg = np.load(os.path.join(GOLDEN, "scene_64x64_4spp_avg.npy"))
    g_rgb = np.load(os.path.join(GOLDEN, "scene_64x64_4spp_rgb8.npy"))
    set_options(room.ds)
    got = room.ds.render_lens(room.cam, sqt.Lens(jitter=0), 4, 1, 64, 64)
    assert np.array_equal(ibits(got.avg), ibits(g_avg)) and np.array_equal(got.rgb.cpu().numpy(), g_rgb)
    avg, rgb = room.ds.render_rows(room.cam, 4, 64, 64)
    assert same_exact(got.avg, avg) and same_exact(got.rgb, rgb)
    # and of a shard, under a depth and a sky
    try:
        set_options(room.ds, sky=SR.GRADIENT, depth=4)
        got = room.ds.render_lens(room.cam, sqt.Lens(jitter=0), 3, 1, 40, 72, shard=(2, 1, 3))
        avg, rgb = room.ds.render_rows(room.cam, 3, 40, 72, shard=(2, 1, 3))
        assert same_exact(got.avg, avg) and same_exact(got.rgb, rgb)
    finally:
        set_options(room.ds)


def test_a_ray_per_sample_gives_the_masked_calls_moments(sqt, room):
    set_options(room.bds)
    got = room.bds.render_lens(room.cam, sqt.Lens(jitter=0), S, S, W, H, want_sum2=True)
    B = buffers(W, H)
    masked(room.bds, room.cam, S, W, H, 0, S, B, np.ones((W, H), np.uint8))
    b = host(B)
    assert (b["sums2"] != 0).any()
    assert np.array_equal(ibits(got.sum2), ibits(b["sums2"])) and np.array_equal(ibits(got.sum), ibits(b["sums"]))
    assert np.array_equal(ibits(got.avg), ibits(b["avg"])) and np.array_equal(got.rgb.cpu().numpy(), b["rgb"])


def test_frames_do_not_depend_on_the_batching(sqt, room):
    set_options(room.bds)
    lens = sqt.Lens(1.0, 0.05, 2.5)
    w, h, s_, r_ = 40, 72, 12, 6
    rows = len(DR.shard_rows(w, (2, 0, 3)))
    p = rows * h
    whole = room.bds.render_lens(room.cam, lens, s_, r_, w, h, shard=(2, 0, 3), want_sum2=True)
    assert (whole.sum != 0).any()
    for nb in (1, 2, 4, 5):
        nbytes = room.lens.work_bytes(p, nb)
        assert len(room.lens.plan(p, 0, r_, nbytes)) == -(-r_ // nb)
        got = room.bds.render_lens(room.cam, lens, s_, r_, w, h, shard=(2, 0, 3), want_sum2=True, work_mb=(nbytes + 15) / 2 ** 20)
        assert same_exact(tuple(got), tuple(whole)), nb
    a = room.bds.render_lens(room.cam, lens, s_, r_, w, h, shard=(2, 0, 3), r_range=(0, 1), want_sum2=True, work_mb=room.lens.work_bytes(p, 1) / 2 ** 20)
    b = room.bds.render_lens(room.cam, lens, s_, r_, w, h, shard=(2, 0, 3), r_range=(1, 6), sums=(a.sum, a.sum2), work_mb=room.lens.work_bytes(p, 2) / 2 ** 20)
    assert same_exact(tuple(b), tuple(whole))
    # anti-aliasing does something: the jittered frame is not the plain one
    plain = room.bds.render_lens(room.cam, sqt.Lens(jitter=0), s_, r_, w, h, shard=(2, 0, 3))
    assert not same_exact(plain.avg, whole.avg)


# ---- 5. the stream promise: tests/test_gpu_streams_lens.py.  It makes streams of its own, and tests/test_gpu_streams.py's control of the
# ---- rig depends on how many streams the process has made before it, so that module has to run first ---------------------------------

# ---- 6. refusals on the device ---------------------------------------------------------------------------------------------
def test_refusals_leave_every_buffer_as_it_was(sqt, room):
    torch = room.torch
    L = room.lens.lib()
    set_options(room.ds)
    B = buffers(W, H)
    nbytes = room.lens.work_bytes(P, 8)
    work = torch.full((nbytes + 64,), 0x3C, dtype=torch.uint8, device="cuda:0")
    sh = sqt.Shard(W, 0, 1)

    def call(scene=room.ds._h, lens=(1.0, 0.0, 1.0), S_=S, R=4, r=(0, 4), w=W, h=H, shard=sh, work_ptr=None, work_bytes=nbytes, **ptr):
        a = {"sum": B["sums"].data_ptr(), "sum2": B["sums2"].data_ptr(), "avg": B["avg"].data_ptr(), "rgb": B["rgb"].data_ptr(), **ptr}
        ln = room.lens.Lens.__new__(room.lens.Lens)
        C.Structure.__init__(ln, *lens)
        rc = L.sq_lens_render_device(scene, C.byref(room.cam), C.byref(ln), S_, R, r[0], r[1], w, h, shard,
                                     work.data_ptr() if work_ptr is None else work_ptr, work_bytes, a["sum"], a["sum2"], a["avg"], a["rgb"], None)
        return rc, L.sq_lens_last_error().decode()

    cases = [(dict(scene=None), "null argument"), (dict(sum=None), "null argument"), (dict(R=3), "must divide"), (dict(r=(0, 5)), "bad sub-ray range"),
             (dict(r=(2, 2)), "bad sub-ray range"), (dict(lens=(1.5, 0.0, 1.0)), "jitter"), (dict(lens=(float("nan"), 0.0, 1.0)), "jitter"),
             (dict(lens=(1.0, -1.0, 1.0)), "aperture"), (dict(lens=(1.0, 0.1, 0.0)), "focus"), (dict(lens=(1.0, 0.1, float("inf"))), "focus"),
             (dict(shard=sqt.Shard(2, 3, 3)), "bad shard"), (dict(work_bytes=room.lens.work_bytes(P, 1) - 1), "too small"),
             (dict(work_ptr=work.data_ptr() + 8), "16-byte aligned"), (dict(sum2=B["sums"].data_ptr() + 12), "d_sum and d_sum2 overlap"),
             (dict(avg=B["sums2"].data_ptr()), "d_sum2 and d_avg overlap"), (dict(rgb=work.data_ptr() + 16), "d_rgb and d_work overlap"),
             (dict(sum=work.data_ptr() + nbytes - 16), "d_sum and d_work overlap")]
    for kw, message in cases:
        rc, err = call(**kw)
        assert rc != 0 and message in err, (kw, err)
    # the two kernels' own entry points
    o = torch.full((4, P, 3), 9.0, dtype=torch.float32, device="cuda:0")
    sd = torch.full((4, P), 9, dtype=torch.int64, device="cuda:0")
    ln = sqt.Lens()
    assert L.sq_lens_rays_device(0, C.byref(room.cam), C.byref(ln), S, 4, 0, 4, W, H, sh, o.data_ptr(), o.data_ptr() + 12, sd.data_ptr(), None) != 0
    assert "d_org and d_dir overlap" in L.sq_lens_last_error().decode()
    assert L.sq_lens_fold_device(0, P, S, 0, 4, o.data_ptr(), o.data_ptr() + 12 * P * 4 - 12, None, None, None, None) != 0
    assert "d_part and d_sum overlap" in L.sq_lens_last_error().decode()
    with pytest.raises(sqt.SquiglyError, match="too small"):
        room.ds.render_lens(room.cam, ln, S, 4, W, H, work_mb=1e-3)
    torch.cuda.synchronize()
    b = host(B)
    from masked_calls import SENT
    assert all((b[k] == SENT[k]).all() for k in ("sums", "sums2", "avg", "rgb"))
    assert (work == 0x3C).all() and (o == 9.0).all() and (sd == 9).all()


def test_the_querys_refusal_is_passed_through(sqt, room):
    """A tree too tall for the wavefront form: sq_raytrace_rays_device refuses the first batch, and sq_lens_render_device returns its
    message; no output buffer is written.  The per-lane form takes the same scene."""
    torch = room.torch
    _, cd = (t.cpu().numpy().reshape(-1, 3) for t in room.ds.camera_rays(room.cam, W, H))
    axis, side = TP.near_side(cd)
    ps = TP.full_stack(room.bright.bih, 200, axis, side)
    ds = sqt.DeviceScene(ps, 0)
    try:
        B = buffers(W, H)
        with pytest.raises(sqt.SquiglyError, match="BIH height 200 needs"):
            ds.render_lens(room.cam, sqt.Lens(), S, 4, W, H, sums=(B["sums"], B["sums2"]))
        torch.cuda.synchronize()
        from masked_calls import SENT
        b = host(B)
        assert (b["sums"] == SENT["sums"]).all() and (b["sums2"] == SENT["sums2"]).all()
        ds.set_option("variant", 1)                                  # the padding is transparent: the room's own frame
        tall = ds.render_lens(room.cam, sqt.Lens(*LR.LENSES["both"]), S, 8, W, H, want_sum2=True)
        assert_frame(tall, want_frame("both", 8, "depth3"), "tall tree, per-lane form")
    finally:
        ds.close()


# ---- 7. the command line -----------------------------------------------------------------------------------------------
def test_cli_aa_frame_is_render_lens(sqt, room, tmp_path, monkeypatch):
    from PIL import Image
    cli = importlib.import_module("squigly-trace_amd.cli")
    monkeypatch.chdir(ROOT)                                          # the reference's default obj and camera paths are relative
    out = str(tmp_path / "aa.png")
    assert cli.main(["-s", "8", "-d", "24,32", "-p", out, "--aa", "--subrays", "4"]) == 0
    set_options(room.ds)
    want = room.ds.render_lens(room.cam, sqt.Lens(), 8, 4, 24, 32).rgb.cpu().numpy()
    assert np.array_equal(np.array(Image.open(out).convert("RGB")), want) and want.any()
    out2 = str(tmp_path / "dof.png")
    assert cli.main(["-s", "4", "-d", "24,32", "-p", out2, "--aperture", "0.1", "--focus", "3", "--depth", "2", "--sky", "0.5,0.5,1"]) == 0
    try:
        set_options(room.ds, sky=((0.5, 0.5, 1.0), (0.5, 0.5, 1.0)), depth=2)
        want2 = room.ds.render_lens(room.cam, sqt.Lens(0.0, 0.1, 3.0), 4, 4, 24, 32).rgb.cpu().numpy()
    finally:
        set_options(room.ds)
    assert np.array_equal(np.array(Image.open(out2).convert("RGB")), want2)
    assert np.array_equal(sqt.render_lens_rgb8(room.c.bih, room.cam, 8, (24, 32), subrays=4), want)
