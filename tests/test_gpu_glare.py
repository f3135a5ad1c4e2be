"""sq_denoise_glare_device on the GPU: every bit of the result (NaN = NaN) against the numpy restatement (tests/glare_restatement.py) at
the sizes where the kernels' indexing can go wrong, in both forms of the down kernels and both lane forms of the composite, and the
drivers on top (sqt.Film(glare=, balance=), Temporal(film=), render_sequence(film=), the command line's --bloom)."""
import importlib
import os

import numpy as np
import pytest

import film_restatement as FR
import glare_restatement as R
import temporal_room as TR
from bitcmp import same
from conftest import DATA
from guarded_alloc import GUARD, guarded, untouched     # (behind d_out and behind the workspace)

pytestmark = pytest.mark.gpu
f32 = np.float32
# 1 x 1, one row, one column; 3 x 5 (odd both ways: every level clamps); 16 x 16 (one direct tile's worth of level 0, and a tiled
# workgroup's tile exactly at level -1 / 2); 17 x 33 and 31 x 32 (one over and one under a tile); 33 x 130 (level 0 is 17 x 65: over the
# 64 lanes of a direct row segment and over a tiled tile, both ways); 37 x 70, which reaches 1 x 1 at level 6, so that levels = 8 runs
# two 1 x 1 -> 1 x 1 steps
SIZES = [(1, 1), (1, 2), (2, 1), (3, 5), (16, 16), (17, 33), (31, 32), (33, 130), (37, 70)]
SIZE_IDS = [f"{r}x{c}" for r, c in SIZES]
LEVELS = (0, 1, 2, 3, 8)
SETTINGS = dict(gain=(1.5, 1.0, 0.6), threshold=0.5, ceiling=8.0, spread=0.6, strength=0.3)


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def dn(sqt, torch):
    mod = importlib.import_module("squigly-trace_amd.denoise")
    mod.lib()
    return mod


@pytest.fixture(scope="module")
def fm(sqt, torch):
    return importlib.import_module("squigly-trace_amd.film")


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(torch, dn, px, skip, levels, form, exposure, in_place=False, **settings):
    """One call over px placed `skip` floats into its allocation, with a NaN-poisoned workspace of exactly the bytes the call needs and
    guards behind the result and the workspace; returns the result on the host."""
    rows, cols = px.shape[:2]
    src, src_whole = guarded(torch, px.shape, skip, -555.0)
    src.copy_(torch.from_numpy(px))
    out, out_whole = (src, src_whole) if in_place else guarded(torch, px.shape, skip, -777.0)
    need = dn.glare_work_bytes(rows, cols, levels)
    assert need == R.work_bytes(rows, cols, levels) and (need > 0) == (levels > 0)
    work_whole = torch.full((need // 4 + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    work = work_whole.view(torch.uint8)[:need] if need else None
    assert src.data_ptr() % 16 == 4 * skip % 16 and out.data_ptr() % 16 == 4 * skip % 16
    got = dn.glare(src, exposure=exposure, levels=levels, form=form, out=out, work=work, **settings)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    n = rows * cols * 3
    assert untouched(out_whole, skip, n, -555.0 if in_place else -777.0), "the guard around d_out"
    assert untouched(work_whole, 0, need // 4, float("nan")), "the guard behind the workspace"
    if not in_place:
        assert same(src.cpu().numpy(), px), "d_color"
    return got.cpu().numpy()


@pytest.mark.parametrize("rows, cols", SIZES, ids=SIZE_IDS)
def test_glare_is_the_restatement_in_every_form(torch, dn, rows, cols):
    """The value table and a random frame, both with NaN, inf and negative pixels, at levels 0, 1, 2, 3 and 8: forms 1 and 2 and the
    chosen one give the restatement's bits, with d_color as allocated (four pixels a lane in the composite) and one float into its
    allocation (one pixel a lane), under an exposure given as a number or as a device float, and in place."""
    frames = [R.value_frame(rows, cols, 200 + rows), R.random_frame(rows, cols, 300 + cols)]
    if rows * cols >= 1000:
        assert all(np.isnan(f).any() and np.isinf(f).any() and (f < 0).any() for f in frames)
    e = 0.7
    e_dev = dev(torch, np.array([e], f32))
    for i, px in enumerate(frames):
        for levels in LEVELS:
            want = R.glare(px, e, levels=levels, **SETTINGS)
            if levels and rows * cols >= 1000:
                assert not same(want, R.glare(px, e, levels=0, **SETTINGS))
            for form in (1, 2, 0):
                for skip in (0, 1):
                    exposure = e_dev if (form + skip + i) % 2 else e
                    got = run(torch, dn, px, skip, levels, form, exposure, **SETTINGS)
                    assert same(got, want), (rows, cols, i, levels, form, skip, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
            for skip in (0, 1):
                got = run(torch, dn, px, skip, levels, 0, e_dev, in_place=True, **SETTINGS)
                assert same(got, want), (rows, cols, i, levels, "in place", skip)


def test_many_tiles_and_a_ragged_edge(torch, dn):
    """300 x 700: level 0 is 150 x 350, which is 10 x 22 tiled workgroups with a ragged edge both ways and 38 x 6 direct ones."""
    px = R.random_frame(300, 700, 9)
    e_dev = dev(torch, np.array([1.3], f32))
    want = R.glare(px, 1.3, levels=5, **SETTINGS)
    for form, skip in ((1, 0), (2, 0), (0, 1), (2, 1)):
        got = run(torch, dn, px, skip, 5, form, e_dev if form else 1.3, **SETTINGS)
        assert same(got, want), (form, skip, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
    # leading dimensions are rows, an allocated result and an allocated workspace, a form by name
    two = np.stack([px[:150], px[150:]])
    got = dn.glare(dev(torch, two), exposure=1.3, levels=5, form="tiled", **SETTINGS)
    assert tuple(got.shape) == two.shape and same(got.cpu().numpy().reshape(300, 700, 3), want)
    E = dn.N.SquiglyError
    src = dev(torch, px)
    with pytest.raises(E, match="out must be"):
        dn.glare(src, out=src[:, :5])
    with pytest.raises(E, match="exposure must be"):
        dn.glare(src, exposure=torch.ones(2, device="cuda"))
    with pytest.raises(E, match="work holds 16 bytes"):
        dn.glare(src, work=torch.empty(16, dtype=torch.uint8, device="cuda"))
    with pytest.raises(E, match="work must be a contiguous torch.uint8 tensor"):
        dn.glare(src, work=torch.empty(1 << 20, dtype=torch.float32, device="cuda"))
    with pytest.raises(E, match="d_color and d_out overlap"):
        dn.glare(src[:299], out=src[1:])                  # shifted by a row: not the allowed d_out == d_color


def test_constant_frame_anchor_on_the_device(torch, dn):
    """A frame of constant 2.0 under e = 1, gain = 1, threshold = 1, ceiling = 4, levels = 3, spread = 0.5 and strength = 0.25 comes out
    as exactly 2.4375 in every pixel, at every size and in every form."""
    for rows, cols in ((1, 1), (1, 2), (3, 5), (17, 33), (37, 70)):
        px = np.full((rows, cols, 3), 2.0, f32)
        for form in (1, 2, 0):
            got = run(torch, dn, px, form % 2, 3, form, 1.0, gain=(1.0, 1.0, 1.0), threshold=1.0, ceiling=4.0, spread=0.5, strength=0.25)
            assert (got == f32(2.4375)).all(), (rows, cols, form)


# ---- the room ----
@pytest.fixture(scope="module")
def scene(sqt, torch, product_scene):
    bih, _, _ = product_scene
    ds = sqt.DeviceScene(bih, 0)
    yield ds
    torch.cuda.synchronize()
    ds.close()


GLARE = dict(threshold=0.25, ceiling=4.0, levels=4, spread=0.7, strength=0.4)


def room_frames(sqt, scene, n_frames, spp=4):
    cams = [sqt.camera_from_text(t) for t in TR.CAMERA_TEXTS[:n_frames]]
    return [scene.render_rows(cam, spp, TR.W, TR.H, want_rgb=False)[0] for cam in cams]


def test_a_glare_of_strength_zero_is_the_plain_film(sqt, torch, scene):
    """Film(glare=Glare(strength=0)) gives the bytes of the plain film under the same curve: the multiply by 1 in develop is exact, and
    x + 0 * U is x but for the sign of a zero, which no curve's byte shows."""
    (avg,) = room_frames(sqt, scene, 1)
    avg = avg * 3.0
    for spec in (dict(curve="filmic"), dict(curve="reinhard", white=4.0, exposure=2.0), dict(curve="atan", auto=dict(key=0.3)), dict(curve="linear", dither=True)):
        plain = sqt.Film(**spec)(avg).cpu().numpy()
        zero = sqt.Film(glare=sqt.Glare(strength=0.0), **spec)(avg).cpu().numpy()
        none = sqt.Film(balance=(1.0, 1.0, 1.0), **spec)(avg).cpu().numpy()
        assert plain.any() and np.array_equal(zero, plain) and np.array_equal(none, plain), spec
        assert not np.array_equal(sqt.Film(glare=sqt.Glare(**GLARE), **spec)(avg).cpu().numpy(), plain), spec


def test_film_with_glare_and_balance_over_three_room_frames(sqt, torch, fm, O, scene):
    """Film(curve="filmic", glare=, balance=, auto=) over three frames of the room under a moving camera, each scaled differently:
    bytes and exposure state equal the restated chain -- the meter sees the frame as it is, the curve sees the glare's."""
    frames = [f * s for f, s in zip(room_frames(sqt, scene, 3), (1.0, 6.0, 0.125))]
    torch.cuda.synchronize()
    host = [f.cpu().numpy() for f in frames]
    auto = dict(key=0.18, permille=900, rate=0.5)
    spec = dict(curve="filmic", lut=fm.srgb_lut(256), dither=True)
    balance = (1.25, 1.0, 0.75)
    want = R.chain(O, host, spec, auto, GLARE, balance)
    plain = FR.chain(O, host, spec, auto)
    film = sqt.Film(auto=auto, glare=sqt.Glare(**GLARE), balance=balance, **spec)
    for i, f in enumerate(frames):
        got = film(f).cpu().numpy()
        assert got.dtype == np.uint8 and np.array_equal(got, want[i][0]), (i, int((got != want[i][0]).sum()))
        assert film.exposure_state == float(want[i][1]) == float(plain[i][1])          # the glare does not move the meter
        assert not np.array_equal(want[i][0], plain[i][0])
    # balance alone: levels = 0
    only = sqt.Film(curve="filmic", exposure=2.0, balance=balance)(frames[0]).cpu().numpy()
    assert np.array_equal(only, R.chain(O, host[:1], dict(curve="filmic", exposure=2.0), None, None, balance)[0][0])


def test_temporal_and_sequence_take_a_film_with_glare(sqt, torch, O, product_scene, scene):
    """Temporal(film=Film(glare=)): step's rgb is the restated film image of step's avg; render_sequence(film=) yields those images."""
    cams = [sqt.camera_from_text(t) for t in TR.CAMERA_TEXTS[:3]]
    spec, auto = dict(curve="reinhard", white=4.0), dict(rate=0.5)
    make = lambda: sqt.Film(auto=auto, glare=sqt.Glare(**GLARE), **spec)                     # noqa: E731
    filmed = sqt.Temporal(scene, TR.W, TR.H, 4, film=make())
    avgs, images = [], []
    for cam in cams:
        r = filmed.step(cam)
        torch.cuda.synchronize()
        avgs.append(r[0].cpu().numpy())
        images.append(r[3].cpu().numpy())
    want = R.chain(O, avgs, spec, auto, GLARE)
    for i in range(3):
        assert np.array_equal(images[i], want[i][0]), i
    seq = list(sqt.render_sequence(product_scene[0], cams, 4, (TR.W, TR.H), film=make()))
    assert len(seq) == 3 and all(np.array_equal(s, i) for s, i in zip(seq, images))


def read_png(path):
    """The (rows, cols, 3) uint8 image of a file written by the package's write_png: 8-bit RGB, one IDAT, filter 0 on every row."""
    import struct
    import zlib
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, {}
    while pos < len(data):
        (n,), tag = struct.unpack(">I", data[pos:pos + 4]), data[pos + 4:pos + 8]
        chunks[tag] = chunks.get(tag, b"") + data[pos + 8:pos + 8 + n]
        pos += 12 + n
    cols, rows, depth, colour, _, _, interlace = struct.unpack(">IIBBBBB", chunks[b"IHDR"])
    assert (depth, colour, interlace) == (8, 2, 0)
    raw = np.frombuffer(zlib.decompress(chunks[b"IDAT"]), np.uint8).reshape(rows, 1 + 3 * cols)
    assert (raw[:, 0] == 0).all()
    return raw[:, 1:].reshape(rows, cols, 3).copy()


def test_cli_bloom(sqt, tmp_path, monkeypatch):
    """The files --sequence --film filmic --bloom writes hold, byte for byte, render_sequence(film=)'s images for the film the flags
    stand for, and differ from the files of the same command without --bloom."""
    cli = importlib.import_module("squigly-trace_amd.cli")
    seq = tmp_path / "move.cams"
    seq.write_text("".join(t.decode() for t in TR.CAMERA_TEXTS[:2]))
    monkeypatch.chdir(os.path.dirname(DATA))
    bih = sqt.BIH(sqt.Mesh.from_obj(os.path.join(DATA, "scene.obj"), DATA))
    size = ["-s", "4", "-d", f"{TR.W},{TR.H}"]
    base = ["--sequence", str(seq), "--film", "filmic", "--exposure", "4"]
    bloom = ["--bloom", "0.5", "--bloom-threshold", "0.25", "--bloom-levels", "4", "--white-balance", "1.25,1,0.75"]
    out, plain_out = str(tmp_path / "bloom.png"), str(tmp_path / "plain.png")
    assert cli.main(base + bloom + size + ["-p", out]) == 0 and cli.main(base + size + ["-p", plain_out]) == 0
    a = cli.parse_args(base + bloom + size)
    film = cli.film_of(a)
    assert film.glare == sqt.Glare(threshold=0.25, ceiling=4.0, levels=4, strength=0.5) and film.balance == (1.25, 1.0, 0.75)
    want = list(sqt.render_sequence(bih, a.sequence, 4, (TR.W, TR.H), temporal=False, film=film))       # no --temporal: each frame on its own
    got = [read_png(p) for p in cli.view_paths(out, 2)]
    plain = [read_png(p) for p in cli.view_paths(plain_out, 2)]
    for i in range(2):
        assert np.array_equal(got[i], want[i]) and got[i].any() and not np.array_equal(got[i], plain[i]), i
