"""libsquigly_denoise.so on the GPU: colour and variance bit for bit (NaN = NaN) against the numpy restatement
(tests/denoise_restatement.py), in every kernel form, at the shapes where indexing can go wrong; the variance kernel on the moments
of a real masked call; the stream promise on a non-blocking side stream; and the Python layers on top (guides, denoise_frame,
render_adaptive, the CLI)."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import denoise_restatement as R
import stream_harness as SH
from bitcmp import same
from conftest import DATA, ROOT
from denoise_room import room
from masked_calls import buffers, masked

pytestmark = pytest.mark.gpu
f32 = np.float32
FORMS = (0, 1, 2)                    # auto, direct, tiled
FORM_IDS = ["auto", "direct", "tiled"]
SIGMA_P = 0.05
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


def inputs(rows, cols, seed):
    key = ("in", rows, cols, seed)
    if key not in _CACHE:
        _CACHE[key] = R.synthetic(rows, cols, seed)
    return _CACHE[key]


def reference(key, color, tri, nrm, pnt, var, **params):
    """The restatement's (out, out_var), computed once per key and shared by the forms."""
    if key not in _CACHE:
        _CACHE[key] = R.denoise(color, tri, nrm, pnt, var, **{"sigma_p": SIGMA_P, **params})
    return _CACHE[key]


def on_gpu(torch, dn, color, tri, nrm, pnt, var, form, out=None, **params):
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    got, got_var = dn.denoise(dev(color), dev(tri), dev(nrm), dev(pnt), var=dev(var), out=out, form=form, **{"sigma_p": SIGMA_P, **params})
    torch.cuda.synchronize()
    return got.cpu().numpy(), None if got_var is None else got_var.cpu().numpy()


def assert_same(got, want, label):
    for name, g, w in (("colour", got[0], want[0]), ("variance", got[1], want[1])):
        if w is None:
            assert g is None, (label, name)
            continue
        assert same(g, w), (label, name, int((~((g.view(np.uint32) == w.view(np.uint32)) | (np.isnan(g) & np.isnan(w)))).sum()), g.shape)


# (rows, cols, passes): 1 x 1; one row, one column (wider than a wave, a tile and a half); smaller than any tile; step 16 reaches past
# the rows; a multiple of no tile; step 128 leaves only the centre row of taps
SHAPES = [(1, 1, 2), (1, 70, 3), (70, 1, 3), (3, 5, 2), (17, 70, 5), (37, 53, 3), (130, 33, 8)]


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("rows, cols, passes", SHAPES, ids=[f"{r}x{c}p{p}" for r, c, p in SHAPES])
def test_shapes(torch, dn, rows, cols, passes, form):
    color, var, tri, nrm, pnt = inputs(rows, cols, seed=rows * 1000 + cols)
    if rows * cols == 1:
        tri = np.zeros((1, 1), np.int32)                        # the one pixel is valid
    want = reference(("shape", rows, cols, passes), color, tri, nrm, pnt, var, passes=passes)
    assert_same(on_gpu(torch, dn, color, tri, nrm, pnt, var, form, passes=passes), want, (rows, cols, passes, form))


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_without_variance(torch, dn, form):
    color, _, tri, nrm, pnt = inputs(37, 53, seed=5)
    want = reference("novar", color, tri, nrm, pnt, None, passes=4)
    assert want[1] is None
    assert_same(on_gpu(torch, dn, color, tri, nrm, pnt, None, form, passes=4), want, form)


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("k", [0, 8])
def test_normal_squarings(torch, dn, k, form):
    color, var, tri, nrm, pnt = inputs(21, 40, seed=6)
    want = reference(("squarings", k), color, tri, nrm, pnt, var, passes=3, normal_squarings=k)
    assert_same(on_gpu(torch, dn, color, tri, nrm, pnt, var, form, passes=3, normal_squarings=k), want, (k, form))


@pytest.mark.parametrize("passes", [1, 4])
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_in_place(torch, dn, form, passes):
    """d_out == d_color and d_out_var == d_var: the inputs are read by the pre-pass alone."""
    color, var, tri, nrm, pnt = inputs(37, 53, seed=7)
    want = reference(("inplace", passes), color, tri, nrm, pnt, var, passes=passes)
    c, v = torch.from_numpy(color.copy()).cuda(), torch.from_numpy(var.copy()).cuda()
    out, out_var = dn.denoise(c, torch.from_numpy(tri).cuda(), torch.from_numpy(nrm).cuda(), torch.from_numpy(pnt).cuda(), var=v, out=(c, v),
                              form=form, passes=passes, sigma_p=SIGMA_P)
    torch.cuda.synchronize()
    assert out.data_ptr() == c.data_ptr() and out_var.data_ptr() == v.data_ptr()
    assert_same((c.cpu().numpy(), v.cpu().numpy()), want, (form, passes))


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("what", ["inf_colour", "nan_normal", "nan_variance", "negative_variance", "all_background"])
def test_special_values(torch, dn, what, form):
    """Values are not checked: an inf, a NaN or a negative number spreads exactly as the expressions say (0 * inf is a NaN)."""
    color, var, tri, nrm, pnt = (a.copy() for a in inputs(19, 37, seed=8))
    tri[9, 18] = tri[9, 19] = 3                                  # the special pixel and a neighbour are valid
    if what == "inf_colour":
        color[9, 18, 1] = np.inf
    elif what == "nan_normal":
        nrm[9, 18, 0] = np.nan
    elif what == "nan_variance":
        var[9, 18] = np.nan
    elif what == "negative_variance":
        var[8:11, 17:20] = -1.0                                  # sqrt of a negative blur: sd is NaN there
    else:
        tri[:] = -1
    want = reference(("special", what), color, tri, nrm, pnt, var, passes=3)
    if what == "inf_colour":
        assert np.isnan(want[0]).any()                           # a weight of zero times inf
    if what == "all_background":
        assert same(want[0], color) and same(want[1], var)
    assert_same(on_gpu(torch, dn, color, tri, nrm, pnt, var, form, passes=3), want, (what, form))


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_workspace_contents_do_not_matter_and_its_end_is_kept(torch, dn, form):
    """A workspace full of NaN bits gives the same result, and the bytes behind work_bytes come back untouched."""
    rows, cols, passes, guard = 37, 53, 3, 4096
    color, var, tri, nrm, pnt = inputs(rows, cols, seed=rows * 1000 + cols)
    want = reference(("shape", rows, cols, passes), color, tri, nrm, pnt, var, passes=passes)
    need = dn.workspace_bytes(rows, cols)
    work = torch.full((need + guard,), 0xFF, dtype=torch.uint8, device="cuda")
    t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (color, var, tri, nrm, pnt)]
    out, out_var = torch.empty_like(t[0]), torch.empty_like(t[1])
    P = dn.make_params(sigma_p=SIGMA_P, passes=passes, form=form)
    dn.check(dn.lib().sq_denoise_device(0, rows, cols, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(),
                                        C.byref(P), out.data_ptr(), out_var.data_ptr(), work.data_ptr(), need, None))
    torch.cuda.synchronize()
    assert_same((out.cpu().numpy(), out_var.cpu().numpy()), want, form)
    assert bool((work[need:] == 0xFF).all())
    assert not bool((work[:need] == 0xFF).all())


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_transposed_image_gives_the_transposed_result(torch, dn, form):
    """rows and cols swapped against a transposed input: the kernel is symmetric in y and x, so a stride mix-up shows.  (The taps
    of a pixel are then added in another order, so the comparison is with the restatement of the transposed input.)"""
    color, var, tri, nrm, pnt = inputs(17, 70, seed=17070)
    tr = [np.ascontiguousarray(np.swapaxes(a, 0, 1)) for a in (color, tri, nrm, pnt, var)]
    want = reference("transposed", tr[0], tr[1], tr[2], tr[3], tr[4], passes=5)
    got = on_gpu(torch, dn, tr[0], tr[1], tr[2], tr[3], tr[4], form, passes=5)
    assert got[0].shape == (70, 17, 3)
    assert_same(got, want, form)
    straight = reference(("shape", 17, 70, 5), color, tri, nrm, pnt, var, passes=5)
    assert np.allclose(np.swapaxes(got[0], 0, 1), straight[0], rtol=1e-3, atol=1e-5, equal_nan=True)


# ---- the room: real guides, real moments ----
@pytest.fixture(scope="module")
def scene(sqt, torch, product_scene):
    bih, cam, _ = product_scene
    ds = sqt.DeviceScene(bih, 0)
    yield ds, cam
    torch.cuda.synchronize()
    ds.close()


@pytest.fixture(scope="module")
def room_frame(torch, dn, scene):
    """The 48 x 64 room at 16 spp from one masked call, its variance and its guides, on the device."""
    ds, cam = scene
    w, h = 48, 64
    B = buffers(w, h)
    for t in B.values():
        t.zero_()
    masked(ds, cam, 16, w, h, 0, 16, B, np.ones((w, h), np.uint8))
    var = dn.denoise_variance(B["sums"], B["sums2"], B["counts"])
    g = ds.guides(cam, w, h)
    torch.cuda.synchronize()
    return B, var, g


def test_guides_are_the_oracles(O, oracle_scene, room_frame):
    _, _, g = room_frame
    rm = room(O, oracle_scene)
    assert np.array_equal(g.tri.cpu().numpy(), rm["tri"])
    hit = rm["tri"] >= 0
    assert same(g.point.cpu().numpy(), rm["point"])
    assert np.allclose(g.normal.cpu().numpy()[hit], rm["normal"][hit], atol=1e-6)
    assert not g.normal.cpu().numpy()[~hit].any() and not g.surf.cpu().numpy()[~hit].any()
    assert (g.surf.cpu().numpy()[hit] >= 0).all() and g.surf.shape == g.emit.shape == (48, 64, 3)


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_room_frame(torch, dn, room_frame, form):
    B, var, g = room_frame
    host = [a.cpu().numpy() for a in (B["avg"], g.tri, g.normal, g.point, var)]
    want = reference("room", *host, passes=5)
    got, got_var = dn.denoise(B["avg"], g.tri, g.normal, g.point, var=var, form=form, passes=5, sigma_p=SIGMA_P)
    torch.cuda.synchronize()
    assert_same((got.cpu().numpy(), got_var.cpu().numpy()), want, form)
    assert not same(got.cpu().numpy(), host[0])                  # and it filtered something


def test_variance_of_a_real_masked_call(torch, dn, scene):
    """Counts 0, 1, 8 and 16 in one frame: three masked calls over shrinking masks."""
    ds, cam = scene
    w, h = 40, 72
    rng = np.random.default_rng(12)
    B = buffers(w, h)
    for t in B.values():
        t.zero_()
    m0 = (rng.random((w, h)) < 0.9).astype(np.uint8)
    m1 = m0 & (rng.random((w, h)) < 0.8)
    m2 = m1 & (rng.random((w, h)) < 0.5)
    masked(ds, cam, 16, w, h, 0, 1, B, m0)
    masked(ds, cam, 16, w, h, 1, 8, B, m1)
    masked(ds, cam, 16, w, h, 8, 16, B, m2)
    counts = B["counts"].cpu().numpy()
    assert set(np.unique(counts)) == {0, 1, 8, 16}
    var = dn.denoise_variance(B["sums"], B["sums2"], B["counts"])
    torch.cuda.synchronize()
    want = R.variance(B["sums"].cpu().numpy(), B["sums2"].cpu().numpy(), counts)
    assert same(var.cpu().numpy(), want)
    assert (want[counts == 0] == 0).all() and (want[counts >= 8] > 0).any()


# ---- the stream promise, in the manner of tests/stream_harness.py ----
class GateEnv(SH.Env):
    """The harness's gate and buffers without its scenes: the filter needs none."""

    def __init__(self, torch):
        self.torch, self.dev = torch, torch.device("cuda", 0)
        self.L = SH.Recorder(None)
        self._calibrate()
        self.side = torch.cuda.Stream(device=self.dev)

    def close(self):
        self.torch.cuda.synchronize()


@pytest.mark.parametrize("form", [1, 2], ids=["direct", "tiled"])
def test_side_stream_behind_pending_work(torch, dn, form):
    """One call on a non-blocking side stream whose inputs arrive only behind a gate and whose outputs are poisoned behind it: the
    pre-pass and every pass are ordered on that stream, and params is read before the call returns (it is overwritten right after)."""
    rows, cols, passes = 37, 53, 3
    color, var, tri, nrm, pnt = inputs(rows, cols, seed=rows * 1000 + cols)
    want = reference(("shape", rows, cols, passes), color, tri, nrm, pnt, var, passes=passes)
    env = GateEnv(torch)
    need = dn.workspace_bytes(rows, cols)
    work = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def step(B, sp, called):
        P = dn.make_params(sigma_p=SIGMA_P, passes=passes, form=form)
        dn.check(dn.lib().sq_denoise_device(0, rows, cols, B["color"].data_ptr(), B["var"].data_ptr(), B["tri"].data_ptr(),
                                            B["normal"].data_ptr(), B["point"].data_ptr(), C.byref(P), B["out"].data_ptr(),
                                            B["out_var"].data_ptr(), work.data_ptr(), need, sp))
        called(P)

    def vstep(B, sp, called):
        dn.check(dn.lib().sq_denoise_variance_device(0, rows * cols, B["color"].data_ptr(), B["normal"].data_ptr(), B["tri"].data_ptr(),
                                                     B["v"].data_ptr(), sp))
        called()

    job = ([("color", "in", color), ("var", "in", var), ("tri", "in", tri), ("normal", "in", nrm), ("point", "in", pnt),
            ("out", "out", ((rows, cols, 3), f32)), ("out_var", "out", ((rows, cols), f32)), ("v", "out", ((rows, cols), f32))], [step, vstep])
    try:
        got = SH.drive(env, job, env.side, f"denoise form {form}")
    finally:
        env.close()
    assert_same((got["out"], got["out_var"]), want, form)
    assert same(got["v"], R.variance(color, nrm, tri))           # the variance kernel on the same stream (any numbers are moments to it)


# ---- the layers on top ----
def test_denoise_frame(torch, dn, sqt, O, oracle_scene, scene, room_frame):
    ds, cam = scene
    B, var, g = room_frame
    avg = B["avg"]
    sp = dn.default_sigma_p(ds.bih.bounds)
    plain_out, plain_var = dn.denoise_frame(ds, cam, 48, 64, avg, var=var, demodulate=False)
    direct, direct_var = dn.denoise(avg, g.tri, g.normal, g.point, var=var, sigma_p=sp)
    out, out_var = sqt.denoise_frame(ds, cam, 48, 64, avg, var=var, guides=g)
    torch.cuda.synchronize()
    assert same(plain_out.cpu().numpy(), direct.cpu().numpy()) and same(plain_var.cpu().numpy(), direct_var.cpu().numpy())
    miss = (g.tri < 0).cpu().numpy()
    assert same(out.cpu().numpy()[miss], avg.cpu().numpy()[miss])
    o = out.cpu().numpy()
    assert np.isfinite(o).all() and (out_var.cpu().numpy() >= 0).all()
    assert not same(o, plain_out.cpu().numpy())                  # demodulation filters another signal
    # against the oracle's 1024-sample frame both filtered frames are nearer than the noisy one (figures: DESIGN.md 4.19)
    rm = room(O, oracle_scene)
    hit = rm["tri"] >= 0
    mse = [float((((a.cpu().numpy().astype(np.float64) - rm["ref"])[hit]) ** 2).mean()) for a in (avg, plain_out, out)]
    print(f"mse over hit pixels: noisy {mse[0]:.4f}, filtered {mse[1]:.4f}, demodulated and filtered {mse[2]:.4f}")
    assert mse[1] < mse[0] and mse[2] < mse[0]


def test_render_adaptive_denoise_and_cli(torch, sqt, product_scene, tmp_path, monkeypatch):
    bih, cam, _ = product_scene
    steps = list(sqt.render_adaptive(bih, cam, 16, (48, 64), 0.5, denoise=True))
    plain_steps = list(sqt.render_adaptive(bih, cam, 16, (48, 64), 0.5))
    assert len(steps) == len(plain_steps) + 1
    for a, b in zip(steps, plain_steps):
        assert a[:3] == b[:3] and np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4])
    img, last = steps[-1][3], plain_steps[-1][3]
    assert img.shape == last.shape == (48, 64, 3) and img.dtype == np.uint8 and not np.array_equal(img, last)
    assert np.array_equal(steps[-1][4], plain_steps[-1][4])
    with pytest.raises(ValueError):
        next(sqt.render_adaptive(bih, cam, 16, (48, 64), 0.5, denoise=-2.0))
    cli = importlib.import_module("squigly-trace_amd.cli")
    monkeypatch.chdir(ROOT)
    path = tmp_path / "filtered.png"
    assert cli.main(["-s", "16", "-d", "48,64", "-p", str(path), "--objpath", os.path.join(DATA, "scene.obj"),
                     "-c", os.path.join(DATA, "camera"), "--adaptive", "0.5", "--denoise"]) == 0
    data = path.read_bytes()
    assert data[:8] == b"\x89PNG\r\n\x1a\n" and len(data) > 100


# ---- past 2^32 bytes of records, and more tiles than a launch has blocks ----
def test_large_image_past_32_bit_byte_offsets(torch, dn):
    """16400 x 16384 pixels: a record array is 4.3 GB (the byte offset of a pixel's record passes 2^32 in the last rows), the
    workspace 17 GB, and both forms have about 2^20 tiles against the 2^16 blocks of a launch, so their tile loops run 16 times --
    the small shapes never take that path.  The two forms agree on every bit, and the image's last corner (and its first) equals the
    restatement of that corner, away from the two edges where the corner was cut out of the image."""
    rows, cols, passes = 16400, 16384, 2
    g = torch.Generator(device="cuda").manual_seed(5)
    rnd = lambda *s: torch.rand(*s, generator=g, device="cuda")            # noqa: E731
    yy = torch.arange(rows, device="cuda", dtype=torch.float32)[:, None, None]
    xx = torch.arange(cols, device="cuda", dtype=torch.float32)[None, :, None]
    color = rnd(rows, cols, 3).mul_(4.0)
    var = rnd(rows, cols)
    tri = torch.where(rnd(rows, cols) < 0.3, -1, 9).to(torch.int32)
    normal = rnd(rows, cols, 3).mul_(0.05).add_(torch.tensor([0.0, 0.6, 0.8], device="cuda"))
    point = rnd(rows, cols, 3).mul_(0.01).add_(0.01 * xx * torch.tensor([1.0, 0.0, 0.0], device="cuda")).add_(
        0.01 * yy * torch.tensor([0.0, 0.8, -0.6], device="cuda"))
    outs = []
    for form in (1, 2):
        out, out_var = dn.denoise(color, tri, normal, point, var=var, form=form, passes=passes, sigma_p=SIGMA_P)
        outs.append((out, out_var))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32))
    assert torch.equal(outs[0][1].view(torch.int32), outs[1][1].view(torch.int32))
    assert dn.workspace_bytes(rows, cols) // 4 > 2 ** 32 and rows * cols * 16 > 2 ** 32
    ch, cw, margin = 64, 96, 16                                   # two passes reach 2 + 4 pixels, and the variance blur one more
    for (y0, x0), keep in (((rows - ch, cols - cw), (slice(margin, None), slice(margin, None))), ((0, 0), (slice(0, ch - margin), slice(0, cw - margin)))):
        crop = lambda t: t[y0:y0 + ch, x0:x0 + cw].cpu().numpy()       # noqa: E731
        want = R.denoise(crop(color), crop(tri), crop(normal), crop(point), crop(var), passes=passes, sigma_p=SIGMA_P)
        assert same(crop(outs[0][0])[keep], want[0][keep]) and same(crop(outs[0][1])[keep], want[1][keep]), (y0, x0)
        assert not same(crop(outs[0][0]), crop(color))
