"""libsquigly_temporal.so on the GPU: colour, variance, length and the unpacked block bit for bit (NaN = NaN) against the numpy
restatement (tests/temporal_restatement.py) at the shapes where indexing can go wrong and under cameras that reproject inside the
image, onto each of its borders, outside it and behind the camera; and the driver on top (sqt.Temporal, render_sequence, the CLI)."""
import collections
import importlib
import os

import numpy as np
import pytest

import denoise_restatement as DR
import temporal_restatement as R
import temporal_room as TR
from bitcmp import same, same_exact
from conftest import DATA, ROOT

pytestmark = pytest.mark.gpu
f32 = np.float32
G = collections.namedtuple("G", ["tri", "normal", "point"])
# 1 x 1; one row wider than two waves; smaller than a tile; no multiple of the tile in either direction; whole tiles; the room's size
SIZES = [(1, 1), (1, 130), (5, 7), (17, 67), (64, 64), (48, 64)]
SIZE_IDS = [f"{r}x{c}" for r, c in SIZES]
CAM = ((0, 0, 0), R.IDENTITY)
SIGMA_P = 0.05
_CACHE = {}


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def tp(sqt, torch):
    mod = importlib.import_module("squigly-trace_amd.temporal")
    mod.lib()
    return mod


def previous_cameras(rows, cols):
    """name -> the camera of the previous frame.  The current frame is CAM's; a wall point (depth 4) that CAM sees at column x and
    row y is seen by a camera shifted by dy along y at column x - dy / 4 * rows, and by one shifted by dz along z at row
    y + dz / 4 * cols (the index quirk: the column offset is scaled by the row count)."""
    px, py = 4.0 / rows, 4.0 / cols
    return {"same": CAM,
            "left": ((0, 0.6 * px, 0), R.IDENTITY),                 # column 0 goes to fx = -0.6
            "right": ((0, -0.6 * px, 0), R.IDENTITY),               # the last column to fx = cols - 0.4
            "down": ((0, 0, -0.6 * py), R.IDENTITY),                # row 0 to fy = -0.6
            "up": ((0, 0, 0.6 * py), R.IDENTITY),                   # the last row to fy = rows - 0.4
            "inside": ((0.3, 0.37 * px, -0.21 * py), R.turned(0.01)),
            "outside": ((0, (cols + 1.3) * px, 0), R.IDENTITY),      # every column leaves the image, in front of the camera
            "behind": ((10, 0, 0), R.IDENTITY)}                     # k_0 <= 0 for every point


def near_camera(rows, cols):
    """A previous camera under which most pixels find their history: the generic one, or for a one-row image a sideways step."""
    return previous_cameras(rows, cols)["inside" if rows > 1 and cols > 1 else "left"]


def frame(rows, cols, seed, cam=CAM, noise=0.01):
    key = (rows, cols, seed, repr(cam), noise)
    if key not in _CACHE:
        _CACHE[key] = R.synthetic(rows, cols, seed, cam, noise, background=0.0 if rows * cols == 1 else 0.08)
    return _CACHE[key]


def alpha_of(rows, cols):
    rng = np.random.default_rng(rows * 1000 + cols)
    a = rng.random((rows, cols)).astype(f32)
    a[rng.random((rows, cols)) < 0.2] = 1.0
    a[0, 0] = np.nan                                                 # compares false: leaves a as it is
    return a


def cam_of(sqt, cam):
    pos, rot = R.camera(cam)
    c = sqt.Camera()
    c.pos[:], c.rot[:] = [float(v) for v in pos], [float(v) for v in rot]
    return c


def dev(torch, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def gpu_frame(torch, fr):
    color, var, tri, nrm, pnt = (dev(torch, a) for a in fr)
    return color, var, G(tri, nrm, pnt)


def first_block(torch, tp, fr):
    """The device block of a first frame (no history), and what the call returned."""
    color, var, g = gpu_frame(torch, fr)
    blk = tp.history(*fr[2].shape, 0)
    out = tp.accumulate(color, var, g, None, None, blk, sigma_p=SIGMA_P)
    return blk, out


def assert_result(torch, tp, got, blk, want, label):
    """(out, out_var, out_len) and the unpacked block `blk` against the restatement's result."""
    torch.cuda.synchronize()
    rows, cols = want["len"].shape
    for name, g, w in (("colour", got[0], want["color"]), ("variance", got[1], want["var"])):
        g = g.cpu().numpy()
        bad = ~((g.view(np.uint32) == w.view(np.uint32)) | (np.isnan(g) & np.isnan(w)))
        assert same(g, w), (label, name, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    assert np.array_equal(got[2].cpu().numpy(), want["len"]), (label, "length")
    h = tp.unpack(blk, rows, cols)
    torch.cuda.synchronize()
    for name in R.BLOCK_FIELDS:
        g, w = getattr(h, name).cpu().numpy(), want["block"][name]
        assert (same(g, w) if w.dtype == f32 else np.array_equal(g, w)), (label, "block", name)


@pytest.mark.parametrize("rows, cols", SIZES, ids=SIZE_IDS)
def test_first_frame_gives_the_inputs_back(torch, tp, rows, cols):
    fr = frame(rows, cols, 1)
    blk, out = first_block(torch, tp, fr)
    want = R.accumulate(*fr, None, None)
    assert same(want["color"], fr[0]) and same(want["var"], fr[1]) and (want["len"] == 1).all()
    assert_result(torch, tp, out, blk, want, (rows, cols))
    assert same_exact(out[0], dev(torch, fr[0])) and same_exact(out[1], dev(torch, fr[1]))         # the inputs' own bits, NaN payloads too


@pytest.mark.parametrize("rows, cols", SIZES, ids=SIZE_IDS)
def test_previous_cameras(sqt, torch, tp, rows, cols):
    """A previous block under cameras that project inside, onto every border, outside and behind; with and without d_alpha."""
    cur = frame(rows, cols, 2)
    color, var, g = gpu_frame(torch, cur)
    hit = cur[2] >= 0
    alpha = alpha_of(rows, cols)
    seen = collections.Counter()
    for name, pcam in previous_cameras(rows, cols).items():
        prev = frame(rows, cols, 3, pcam)
        pblk, _ = first_block(torch, tp, prev)
        ok, fx, fy = R.project(pcam, rows, cols, cur[4])
        ok &= hit
        seen.update({"inside": int((ok & (fx >= 0) & (fx < cols - 1) & (fy >= 0) & (fy < rows - 1)).sum()),
                     "fx<0": int((ok & (fx < 0)).sum()), "fx>=cols-1": int((ok & (fx >= cols - 1)).sum()),
                     "fy<0": int((ok & (fy < 0)).sum()), "fy>=rows-1": int((ok & (fy >= rows - 1)).sum()),
                     "outside": int((hit & ~ok).sum()) if name == "outside" else 0, "behind": int((hit & ~ok).sum()) if name == "behind" else 0})
        if name == "behind":
            assert not ok.any()
        for a in (None, alpha):
            nxt = tp.history(rows, cols, 0)
            got = tp.accumulate(color, var, g, cam_of(sqt, pcam), pblk, nxt, alpha=dev(torch, a), sigma_p=SIGMA_P)
            want = R.accumulate(*cur, pcam, R.first_block(*prev), alpha=a, sigma_p=SIGMA_P)
            assert_result(torch, tp, got, nxt, want, (rows, cols, name, a is not None))
            if name == "same" or (name == "inside" and rows > 1 and cols > 1):     # (a forward step takes a one-row image out of sight)
                assert (want["len"] == 2).any(), (name, "no pixel found its history")
    need = ["fx<0", "fx>=cols-1", "fy<0", "fy>=rows-1", "outside", "behind"] + (["inside"] if rows > 1 and cols > 1 else [])
    assert all(seen[k] > 0 for k in need), seen           # every case happens at every size (a 1-wide image has no interior)


@pytest.mark.parametrize("rows, cols", SIZES, ids=SIZE_IDS)
def test_parameters(sqt, torch, tp, rows, cols):
    """Taps at exact equality of both stops (the planes are exact: n_p . n_q = 1 and |pd| is 0 or 2), a previous frame that is all
    background, max_history 1, alpha_min 0 and 1."""
    pcam = near_camera(rows, cols)
    cur, prev = frame(rows, cols, 4, CAM, 0.0), frame(rows, cols, 5, pcam, 0.0)
    color, var, g = gpu_frame(torch, cur)
    pblk, _ = first_block(torch, tp, prev)
    pwant = R.first_block(*prev)
    cases = [dict(cos_n=1.0, sigma_p=2.0), dict(cos_n=1.0, sigma_p=0.0), dict(cos_n=np.nextafter(f32(1), f32(2)), sigma_p=2.0),
             dict(sigma_p=float(np.nextafter(f32(2), f32(0)))), dict(sigma_p=SIGMA_P, max_history=1), dict(sigma_p=SIGMA_P, alpha_min=0.0),
             dict(sigma_p=SIGMA_P, alpha_min=1.0)]
    lens, wants = [], []
    for params in cases:
        params = {k: (float(v) if k != "max_history" else v) for k, v in params.items()}
        nxt = tp.history(rows, cols, 0)
        got = tp.accumulate(color, var, g, cam_of(sqt, pcam), pblk, nxt, **params)
        want = R.accumulate(*cur, pcam, pwant, **params)
        assert_result(torch, tp, got, nxt, want, (rows, cols, params))
        lens.append(want["len"])
        wants.append(want)
    if rows * cols > 1:
        assert (lens[0] == 2).any() and (lens[2] == 1).all()          # equality is accepted; one ulp past it nothing is
        assert (lens[4] == 1).all()                                   # max_history 1
    if rows >= 17:                                                    # |pd| = 2 taps: taken at sigma_p = 2, left out just below it
        assert (lens[0] == 2).sum() >= (lens[3] == 2).sum() > 0 and not same(wants[0]["color"], wants[3]["color"])
    # all background: no tap, the inputs come back
    empty = tuple(a if i != 2 else np.full_like(a, -1) for i, a in enumerate(prev))
    eblk, _ = first_block(torch, tp, empty)
    nxt = tp.history(rows, cols, 0)
    got = tp.accumulate(color, var, g, cam_of(sqt, pcam), eblk, nxt, sigma_p=SIGMA_P)
    want = R.accumulate(*cur, pcam, R.first_block(*empty), sigma_p=SIGMA_P)
    assert (want["len"] == 1).all() and same(want["color"], cur[0])
    assert_result(torch, tp, got, nxt, want, (rows, cols, "all background"))


def moving_cameras(rows, cols, n):
    px, py = 4.0 / rows, 4.0 / cols
    return [((0.02 * i, 0.45 * px * i, -0.3 * py * i), R.turned(0.004 * i)) for i in range(n)]


@pytest.mark.parametrize("rows, cols", SIZES, ids=SIZE_IDS)
def test_chain_of_five_frames(sqt, torch, tp, rows, cols):
    """Five frames through two blocks that take turns, with d_alpha, max_history 3: every frame equals the restatement's chain."""
    cams = moving_cameras(rows, cols, 5)
    frames = [frame(rows, cols, 10 + i, cams[i]) for i in range(5)]
    alphas = [alpha_of(rows, cols) * f32(0.5) for _ in range(5)]
    params = dict(sigma_p=SIGMA_P, max_history=3, alpha_min=0.05)
    want = R.chain(frames, cams, alphas, **params)
    blocks = [tp.history(rows, cols, 0), tp.history(rows, cols, 0)]
    prev, prev_cam = None, None
    for i, fr in enumerate(frames):
        color, var, g = gpu_frame(torch, fr)
        nxt = blocks[i & 1]
        got = tp.accumulate(color, var, g, prev_cam, prev, nxt, alpha=dev(torch, alphas[i]), **params)
        assert_result(torch, tp, got, nxt, want[i], (rows, cols, "frame", i))
        prev, prev_cam = nxt, cam_of(sqt, cams[i])
    if rows > 1 and cols > 1:
        assert want[-1]["len"].max() == 3 and (want[2]["len"] == 3).any()


@pytest.mark.parametrize("rows, cols", SIZES, ids=SIZE_IDS)
def test_in_place(sqt, torch, tp, rows, cols):
    """d_out == d_color and d_out_var == d_var: a thread reads its own pixel before it writes it."""
    pcam = near_camera(rows, cols)
    cur, prev = frame(rows, cols, 6), frame(rows, cols, 7, pcam)
    color, var, g = gpu_frame(torch, cur)
    pblk, _ = first_block(torch, tp, prev)
    nxt = tp.history(rows, cols, 0)
    got = tp.accumulate(color, var, g, cam_of(sqt, pcam), pblk, nxt, out=(color, var), sigma_p=SIGMA_P)
    assert got[0].data_ptr() == color.data_ptr() and got[1].data_ptr() == var.data_ptr()
    assert_result(torch, tp, got, nxt, R.accumulate(*cur, pcam, R.first_block(*prev), sigma_p=SIGMA_P), (rows, cols))


def test_more_tiles_than_blocks(sqt, torch, tp):
    """8200 x 70: 2 x 2050 tiles of 4 rows x 64 columns against the 2048 blocks of a launch, so the kernel's tile loop runs more than
    once -- the small shapes never take that path."""
    rows, cols = 8200, 70
    pcam = ((0, 0.37 * 4.0 / rows, -0.21 * 4.0 / cols), R.IDENTITY)      # sideways by a fraction of a pixel: every row keeps its history
    cur, prev = R.synthetic(rows, cols, 8, CAM, 0.01), R.synthetic(rows, cols, 9, pcam, 0.01)
    color, var, g = gpu_frame(torch, cur)
    pblk, _ = first_block(torch, tp, prev)
    nxt = tp.history(rows, cols, 0)
    got = tp.accumulate(color, var, g, cam_of(sqt, pcam), pblk, nxt, sigma_p=SIGMA_P)
    want = R.accumulate(*cur, pcam, R.first_block(*prev), sigma_p=SIGMA_P)
    assert (want["len"][-4:] == 2).any() and (want["len"][:4] == 2).any()
    assert_result(torch, tp, got, nxt, want, (rows, cols))


def test_python_layer_refusals(sqt, torch, tp):
    fr = frame(5, 7, 1)
    color, var, g = gpu_frame(torch, fr)
    blk, other = tp.history(5, 7, 0), tp.history(5, 7, 0)
    E = tp.N.SquiglyError
    with pytest.raises(E, match="sigma_p is required"):
        tp.accumulate(color, var, g, None, None, blk)
    with pytest.raises(E, match="go together"):
        tp.accumulate(color, var, g, sqt.Camera(), None, blk, sigma_p=SIGMA_P)
    with pytest.raises(E, match="nxt must be"):
        tp.accumulate(color, var, g, None, None, blk[:-16], sigma_p=SIGMA_P)
    with pytest.raises(E, match="var must be"):
        tp.accumulate(color, var[:, :6], g, None, None, blk, sigma_p=SIGMA_P)
    with pytest.raises(E, match="d_prev and d_next overlap"):
        tp.accumulate(color, var, g, sqt.Camera(), blk, blk, sigma_p=SIGMA_P)
    with pytest.raises(E, match="alpha_min"):
        tp.accumulate(color, var, g, None, None, blk, sigma_p=SIGMA_P, alpha_min=2.0)
    with pytest.raises(E, match="hist must be"):
        tp.unpack(blk, 5, 8)
    with pytest.raises(E, match="at least 1"):
        tp.history(0, 7, 0)
    assert other.numel() == tp.history_bytes(5, 7) == 5 * 7 * 48 and other.data_ptr() % 16 == 0


# ---- the room: real guides, the oracle's samples ----
@pytest.fixture(scope="module")
def scene(sqt, torch, product_scene):
    bih, _, _ = product_scene
    ds = sqt.DeviceScene(bih, 0)
    yield ds
    torch.cuda.synchronize()
    ds.close()


def test_room_guides_and_oracle_samples(sqt, torch, tp, O, oracle_scene, scene):
    """Two cameras of the room's sequence: the device's own guides (DeviceScene.guides) and the oracle's 16-sample frames,
    demodulated, with alpha from `reflective`: the second frame against the restatement on the same inputs."""
    seq = TR.sequence(O, oracle_scene)
    cams = [sqt.camera_from_text(t) for t in TR.CAMERA_TEXTS[:2]]
    counts = np.full((TR.W, TR.H), TR.SPP, np.int32)
    frames, alphas, gpu = [], [], []
    for i, cam in enumerate(cams):
        g = scene.guides(cam, TR.W, TR.H)
        torch.cuda.synchronize()
        og = seq["frames"][i]["guides"]
        assert np.array_equal(g.tri.cpu().numpy(), og["tri"]) and same(g.point.cpu().numpy(), og["point"])
        fr = seq["frames"][i]
        hg = dict(og, normal=g.normal.cpu().numpy(), surf=g.surf.cpu().numpy(), emit=g.emit.cpu().numpy())
        x, v, _, _ = TR.demodulate(fr["avg"], DR.variance(fr["sums"], fr["sums2"], counts), hg)
        alpha = tp.frame_alpha(scene, g.tri)
        torch.cuda.synchronize()
        assert same(alpha.cpu().numpy(), og["reflective"])
        frames.append((x, v, og["tri"], hg["normal"], og["point"]))
        alphas.append(og["reflective"])
        gpu.append((dev(torch, x), dev(torch, v), g, alpha))
    sp = importlib.import_module("squigly-trace_amd.denoise").default_sigma_p(scene.bih.bounds)
    want = R.chain(frames, cams, alphas, **dict(R.DEFAULTS, sigma_p=sp))
    blocks = [tp.history(TR.W, TR.H, 0), tp.history(TR.W, TR.H, 0)]
    got0 = tp.accumulate(gpu[0][0], gpu[0][1], gpu[0][2], None, None, blocks[0], alpha=gpu[0][3], sigma_p=sp)
    assert_result(torch, tp, got0, blocks[0], want[0], "room frame 0")
    got1 = tp.accumulate(gpu[1][0], gpu[1][1], gpu[1][2], cams[0], blocks[0], blocks[1], alpha=gpu[1][3], sigma_p=sp)
    assert_result(torch, tp, got1, blocks[1], want[1], "room frame 1")
    hit = frames[1][2] >= 0
    assert (want[1]["len"][hit] == 2).mean() > 0.9 and (want[1]["len"][hit] == 1).any()


# ---- the driver ----
def by_hand(sqt, torch, tp, ds, cam, prev_cam, prev, nxt, f, spp, period, params, dn=None):
    """A Temporal.step written out in the primitive calls."""
    w, h = TR.W, TR.H
    denoise = importlib.import_module("squigly-trace_amd.denoise")
    sums = torch.zeros((w, h, 3), dtype=torch.float32, device="cuda")
    sums2 = torch.zeros((w, h, 3), dtype=torch.float32, device="cuda")
    k0 = (f % period) * spp
    ds.render_rows_masked(cam, spp * period, w, h, k0, k0 + spp, sums, sums2=sums2, want_avg=False, want_rgb=False)
    noisy = sums / float(spp)
    var = denoise.denoise_variance(sums, sums2, torch.full((w, h), spp, dtype=torch.int32, device="cuda"))
    g = ds.guides(cam, w, h)
    ok = ((g.tri >= 0) & (g.surf > 0).all(-1))[..., None]
    x = torch.where(ok, (noisy - g.emit) / torch.where(ok, g.surf, torch.ones_like(g.surf)), noisy)
    ls = (0.25 * g.surf[..., 0] + 0.5 * g.surf[..., 1]) + 0.25 * g.surf[..., 2]
    scale = torch.where(ok[..., 0], ls * ls, torch.ones_like(ls))
    out, out_var, length = tp.accumulate(x, var / scale, g, prev_cam, prev, nxt, alpha=tp.frame_alpha(ds, g.tri), **params)
    if dn is not None:
        out, out_var = denoise.denoise(out, g.tri, g.normal, g.point, var=out_var, **dn)
    return torch.where(ok, out * g.surf + g.emit, out), out_var * scale, length, noisy


@pytest.mark.parametrize("filtered", [False, True], ids=["plain", "denoise"])
def test_step_is_the_primitive_calls(sqt, torch, tp, scene, filtered):
    """Three steps of sqt.Temporal against the same primitive calls made by hand, bit for bit; frame f's noisy mean is
    render_rows_range of its k-range started from zero sums; the frames take different seeds."""
    spp, period = 4, 3
    cams = [sqt.camera_from_text(t) for t in TR.CAMERA_TEXTS[:4]]
    sp = importlib.import_module("squigly-trace_amd.denoise").default_sigma_p(scene.bih.bounds)
    params = dict(alpha_min=0.2, max_history=2, cos_n=0.9, sigma_p=sp)
    t = sqt.Temporal(scene, TR.W, TR.H, spp, period=period, alpha_min=0.2, max_history=2, denoise={"passes": 2} if filtered else None)
    assert t.frames == 0 and t.history is None and t.camera is None and t.params == params
    blocks = [tp.history(TR.W, TR.H, 0), tp.history(TR.W, TR.H, 0)]
    prev, prev_cam, noisies = None, None, []
    for f, cam in enumerate(cams):
        avg, var, length, rgb = t.step(cam)
        want = by_hand(sqt, torch, tp, scene, cam, prev_cam, prev, blocks[f & 1], f, spp, period, params,
                       {"passes": 2, "sigma_p": sp} if filtered else None)
        torch.cuda.synchronize()
        assert same_exact((avg, var, length), want[:3]), f
        assert same_exact(t.noisy, want[3]) and same_exact(t.history, blocks[f & 1])
        assert t.frames == f + 1 and bytes(t.camera) == bytes(cam)
        assert rgb.dtype == torch.uint8 and tuple(rgb.shape) == (TR.W, TR.H, 3) and bool((rgb > 0).any())
        # the noisy frame is the k-range of the (spp * period)-sample frame, from zero sums
        sums = torch.zeros((TR.W, TR.H, 3), dtype=torch.float32, device="cuda")
        k0 = (f % period) * spp
        scene.render_rows_range(cam, spp * period, TR.W, TR.H, k0, k0 + spp, sums, want_avg=False, want_rgb=False)
        torch.cuda.synchronize()
        assert same_exact(t.noisy, sums / float(spp))
        noisies.append(t.noisy)
        prev, prev_cam = blocks[f & 1], cam
    assert int(length.max()) == 2 and int(length.min()) == 1
    # frame 3 is frame 0's sample range again (period 3), frame 1 another: under one camera the first repeats and the second does not
    t.reset()
    assert t.frames == 0 and t.history is None
    for f in range(4):
        t.step(cams[0])
        noisies.append(t.noisy)
    torch.cuda.synchronize()
    assert same_exact(noisies[4], noisies[7]) and not same_exact(noisies[4], noisies[5])
    assert same_exact(noisies[4], noisies[0])


def test_checkpoint_and_resume(sqt, torch, tp, scene):
    """(history, camera, frames) copied away after two steps and passed back in: a new Temporal continues with the same bits."""
    spp = 4
    cams = [sqt.camera_from_text(t) for t in TR.CAMERA_TEXTS[:4]]
    a = sqt.Temporal(scene, TR.W, TR.H, spp, period=8)
    for cam in cams[:2]:
        a.step(cam)
    torch.cuda.synchronize()
    saved = (a.history.cpu().numpy().copy(), sqt.Camera.from_buffer_copy(bytes(a.camera)), a.frames, a.depth, a.sky)
    rest_a = [a.step(cam) for cam in cams[2:]]
    b = sqt.Temporal(scene, TR.W, TR.H, spp, period=8, history=saved[0], camera=saved[1], frames=saved[2], depth=saved[3], sky=saved[4])
    assert b.frames == 2
    rest_b = [b.step(cam) for cam in cams[2:]]
    torch.cuda.synchronize()
    for x, y in zip(rest_a, rest_b):
        assert same_exact(x[:3], y[:3]) and torch.equal(x[3], y[3])
    assert same_exact(a.history, b.history) and int(rest_a[-1][2].max()) == 4
    with pytest.raises(ValueError, match="history must have shape"):
        sqt.Temporal(scene, TR.W, TR.H, spp, history=saved[0][:-48], camera=saved[1], frames=2)
    with pytest.raises(sqt.SquiglyError, match="depth"):
        sqt.Temporal(scene, TR.W, TR.H, spp, depth=2)
    scene.set_depth(2)
    try:
        with pytest.raises(sqt.SquiglyError, match="begun under"):
            b.step(cams[0])
    finally:
        scene.set_depth(3)


def test_render_sequence_and_cli(sqt, torch, product_scene, tmp_path, monkeypatch):
    bih, _, _ = product_scene
    cams = [sqt.camera_from_text(t) for t in TR.CAMERA_TEXTS[:3]]
    acc = list(sqt.render_sequence(bih, cams, 4, (TR.W, TR.H)))
    plain = list(sqt.render_sequence(bih, cams, 4, (TR.W, TR.H), temporal=False))
    assert len(acc) == len(plain) == 3
    assert all(i.shape == (TR.W, TR.H, 3) and i.dtype == np.uint8 for i in acc + plain)
    assert np.array_equal(acc[0], plain[0]) and not np.array_equal(acc[2], plain[2])       # the first frame has no history
    filtered = list(sqt.render_sequence(bih, cams[:2], 4, (TR.W, TR.H), denoise=True))
    assert not np.array_equal(filtered[1], acc[1])
    cli = importlib.import_module("squigly-trace_amd.cli")
    monkeypatch.chdir(ROOT)
    seq = tmp_path / "move.cams"
    seq.write_bytes(b"".join(TR.CAMERA_TEXTS[:3]))
    path = tmp_path / "move.png"
    assert cli.main(["-s", "4", "-d", f"{TR.W},{TR.H}", "-p", str(path), "--objpath", os.path.join(DATA, "scene.obj"),
                     "--sequence", str(seq), "--temporal", "0.2"]) == 0
    for p in cli.view_paths(str(path), 3):
        data = open(p, "rb").read()
        assert data[:8] == b"\x89PNG\r\n\x1a\n" and len(data) > 100
