"""libsquigly_film.so on the GPU: histogram, exposure, bytes and display values bit for bit (NaN = NaN) against the numpy restatement
(tests/film_restatement.py) at the sizes where the kernels' indexing can go wrong, in both forms of the develop kernel, and the
drivers on top (sqt.Film, Temporal(film=), render_adaptive(film=))."""
import importlib
import os

import numpy as np
import pytest

import film_restatement as R
import temporal_room as TR
from bitcmp import same
from conftest import DATA

pytestmark = pytest.mark.gpu
f32 = np.float32
inf = float("inf")
# 1, 3, 3, 4, 5, 255, 256, 257 and 1025 pixels: below, at (2 x 2: one quad, no tail, no loop) and over a lane's four pixels and a
# workgroup's 256 lanes, with every n % 4; then 37 x 70, which holds every edge of the value table several times.  No row or column count but 16 is a multiple of 8.
SIZES = [(1, 1), (1, 3), (3, 1), (2, 2), (1, 5), (5, 51), (16, 16), (257, 1), (25, 41), (37, 70)]
SIZE_IDS = [f"{r}x{c}" for r, c in SIZES]
LUTS = ("none", "two", "srgb")
COMBOS = [("reference", "none", False)] + [(c, t, d) for c in R.CURVES[1:] for t in LUTS for d in (False, True)]


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def fm(sqt, torch):
    mod = importlib.import_module("squigly-trace_amd.film")
    mod.lib()
    return mod


def lut_named(fm, name):
    return {"none": None, "two": np.array([0.25, 0.75], f32), "srgb": fm.srgb_lut(4096)}[name]


def dev(torch, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def offset_tensor(torch, shape, dtype, skip):
    """An uninitialised contiguous tensor of `shape` that starts `skip` elements into its allocation."""
    n = int(np.prod(shape))
    return torch.empty(n + skip, dtype=dtype, device="cuda")[skip:].view(*shape)


def place(torch, a, skip):
    t = offset_tensor(torch, a.shape, torch.float32, skip)
    t.copy_(torch.from_numpy(a))
    return t


@pytest.mark.parametrize("rows, cols", SIZES, ids=SIZE_IDS)
def test_develop_is_the_restatement_in_both_forms(torch, fm, O, rows, cols):
    """Every curve, table and dither setting over the value table; each with d_color one float and d_rgb one byte into their
    allocations (the one-pixel-a-lane form) and with both as the allocator gives them (the four-pixels-a-lane form), with and without
    d_display, under an exposure given as a number or as a device float."""
    px = R.value_table(rows * cols, 100 + rows).reshape(rows, cols, 3)
    if rows * cols >= 1025:
        assert np.isnan(px).any() and np.isinf(px).any() and (px < 0).any() and (px.max(-1) == 0).any()
    narrow_in, wide_in = place(torch, px, 1), place(torch, px, 0)
    assert wide_in.data_ptr() % 16 == 0 and narrow_in.data_ptr() % 16 == 4
    forms = set()
    for i, (curve, lut_name, dither) in enumerate(COMBOS):
        table = lut_named(fm, lut_name)
        e, white = (1.0, inf) if i % 3 == 0 else (0.7, 2.5)
        want_rgb, want_disp = R.develop(O, px, e, curve, white, table, dither)
        lut = dev(torch, table)
        exposure = dev(torch, np.array([e], f32)) if i % 2 else e
        for form, src, skip in (("four", wide_in, 0), ("one", narrow_in, 1)):
            for want_display in (False, True):
                rgb = offset_tensor(torch, px.shape, torch.uint8, skip).fill_(0xA5)
                disp = offset_tensor(torch, px.shape, torch.float32, skip).fill_(-777.0) if want_display else None
                assert rgb.data_ptr() % 4 == skip and (disp is None or disp.data_ptr() % 16 == 4 * skip)
                forms.add((form, src.data_ptr() % 16 == 0 and rgb.data_ptr() % 4 == 0))
                got = fm.develop(src, exposure, curve, white, lut, dither, out=(rgb, disp) if want_display else rgb, want_display=want_display)
                torch.cuda.synchronize()
                label = (rows, cols, curve, lut_name, dither, form, want_display)
                g = (got[0] if want_display else got).cpu().numpy()
                assert np.array_equal(g, want_rgb), (label, np.argwhere(g != want_rgb)[:4].tolist())
                if want_display:
                    assert got[1].data_ptr() == disp.data_ptr() and same(disp.cpu().numpy(), want_disp), label
    assert forms == {("four", True), ("one", False)}


def test_develop_forms_by_each_pointer(torch, fm, O):
    """Which form runs is decided by d_color and d_rgb alone: either one off its alignment takes the one-pixel form, and d_display off
    its own only narrows the four-pixel form's display stores.  All give the restatement's bits; allocated outputs as well."""
    rows, cols = 37, 70
    px = R.value_table(rows * cols, 7).reshape(rows, cols, 3)
    table = fm.srgb_lut(4096)
    want_rgb, want_disp = R.develop(O, px, 1.3, "filmic", inf, table, True)
    lut = dev(torch, table)
    for skip_in, skip_rgb, skip_disp in ((0, 0, 0), (0, 0, 1), (0, 0, 2), (1, 0, 0), (2, 0, 0), (0, 1, 0), (0, 2, 1), (0, 3, 3), (3, 3, 3)):
        src = place(torch, px, skip_in)
        rgb = offset_tensor(torch, px.shape, torch.uint8, skip_rgb).fill_(0xA5)
        disp = offset_tensor(torch, px.shape, torch.float32, skip_disp).fill_(-777.0)
        fm.develop(src, 1.3, "filmic", lut=lut, dither=True, out=(rgb, disp), want_display=True)
        torch.cuda.synchronize()
        assert np.array_equal(rgb.cpu().numpy(), want_rgb) and same(disp.cpu().numpy(), want_disp), (skip_in, skip_rgb, skip_disp)
    rgb, disp = fm.develop(dev(torch, px), 1.3, "filmic", lut=lut, dither=True, want_display=True)
    assert rgb.dtype == torch.uint8 and tuple(rgb.shape) == px.shape and np.array_equal(rgb.cpu().numpy(), want_rgb) and same(disp.cpu().numpy(), want_disp)
    # leading dimensions are rows: [2, rows, cols, 3] is the image of 2 * rows rows, and the dither's rows go on counting
    two = np.stack([px, px[::-1]])
    got = fm.develop(dev(torch, two), 1.3, "filmic", lut=lut, dither=True)
    assert tuple(got.shape) == two.shape
    assert np.array_equal(got.cpu().numpy().reshape(2 * rows, cols, 3), R.develop(O, two.reshape(2 * rows, cols, 3), 1.3, "filmic", inf, table, True)[0])
    E = fm.N.SquiglyError
    with pytest.raises(E, match="d_color and d_display overlap"):
        fm.develop(src := dev(torch, px), curve="linear", out=(rgb, src), want_display=True)
    with pytest.raises(E, match="out image must be"):
        fm.develop(src, out=rgb[:, :5])
    with pytest.raises(E, match="exposure must be"):
        fm.develop(src, exposure=torch.ones(2, device="cuda"))
    with pytest.raises(E, match="lut must be"):
        fm.develop(src, curve="atan", lut=table)
    with pytest.raises(E, match="reference curve"):
        fm.develop(src, lut=lut)


def test_more_quads_than_lanes(torch, fm, O):
    """2100 x 1001 pixels: 525 525 quads against the 2048 x 256 lanes of a launch, so the four-pixel form's loop runs more than once
    and ends in a one-pixel tail; the one-pixel form's loop runs five times.  The linear curve with dither: no arctangent to restate."""
    rows, cols = 2100, 1001
    rng = np.random.default_rng(5)
    px = (rng.random((rows, cols, 3)) * 1.2 - 0.1).astype(f32)
    want = R.develop(O, px, 0.9, "linear", inf, None, True)[0]
    for skip in (0, 1):
        got = fm.develop(place(torch, px, skip), 0.9, "linear", dither=True)
        torch.cuda.synchronize()
        assert np.array_equal(got.cpu().numpy(), want), skip


# ---- the room ----
@pytest.fixture(scope="module")
def scene(sqt, torch, product_scene):
    bih, _, _ = product_scene
    ds = sqt.DeviceScene(bih, 0)
    yield ds
    torch.cuda.synchronize()
    ds.close()


def test_room_anchor(sqt, torch, fm, O, oracle_scene, product_scene, scene):
    """The room at 48 x 64, 4 spp: develop(avg) at its defaults is the rgb of the same render_rows call, and the oracle's."""
    w, h, n = TR.W, TR.H, 4
    avg, rgb = scene.render_rows(product_scene[1], n, w, h)
    got = fm.develop(avg)
    torch.cuda.synchronize()
    ref_avg, ref_rgb, _ = oracle_scene[0].render(oracle_scene[1], n, w, h, threads=min(os.cpu_count() or 1, 8))
    assert same(avg.cpu().numpy(), ref_avg)
    assert np.array_equal(got.cpu().numpy(), rgb.cpu().numpy()) and np.array_equal(got.cpu().numpy(), ref_rgb)
    assert (ref_rgb.sum(-1) > 0).sum() > w * h // 100        # at 4 spp most of the room is still black; the anchor is not all black
    assert np.array_equal(sqt.Film()(avg).cpu().numpy(), ref_rgb)
    rgb2, disp = fm.develop(avg, want_display=True)
    assert np.array_equal(rgb2.cpu().numpy(), ref_rgb) and same(disp.cpu().numpy(), R.develop(O, ref_avg)[1])


# ---- histogram and expose ----
def histogram_images():
    rng = np.random.default_rng(17)
    big = (10.0 ** rng.uniform(-3, 1, (300, 700, 3))).astype(f32)
    big[:120] = 0                                            # black rows: whole waves of slot 0
    big[rng.random((300, 700)) < 0.3] = 0                    # and black pixels among the others
    big[200:230] = big[200, 0]                               # whole waves of one other slot
    return {"1x1": np.array([[[0.5, 0.25, 0.125]]], f32), "1x1 black": np.zeros((1, 1, 3), f32), "every slot": R.slot_image(37, 70, 3),
            "one slot": np.full((37, 70, 3), 0.18, f32), "one slot, 5 waves and a bit": np.full((1, 333, 3), 2.5, f32),
            "all black": np.zeros((37, 70, 3), f32), "300x700": big}


METERS = (dict(), dict(permille=1), dict(permille=1000, key=0.5), dict(permille=900, e_min=0.5, e_max=2.0, rate=0.25, fallback=3.0))


def test_histogram_and_expose_are_the_restatement(torch, fm):
    """Each image's histogram equals numpy.bincount of the restated slots and sums to rows * cols; on each, expose equals the
    restatement without a previous exposure, with one (usable or not), and in place."""
    seen = set()
    for name, img in histogram_images().items():
        want = R.histogram(img)
        assert want.sum() == img.shape[0] * img.shape[1]
        for skip in (0, 1):
            out = torch.full((R.SLOTS,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            got = fm.histogram(place(torch, img, skip), out=out)
            torch.cuda.synchronize()
            assert got.data_ptr() == out.data_ptr() and np.array_equal(out.cpu().numpy().astype(np.int64), want), (name, skip)
        hist = fm.histogram(dev(torch, img))
        assert hist.dtype == torch.int32 and int(hist.sum()) == img.shape[0] * img.shape[1]
        seen |= set(np.nonzero(want)[0].tolist())
        for meter in METERS:
            for prev in (None, 2.0, 0.0, float("nan"), inf):
                want_e = R.expose(want, prev, **meter)
                p = None if prev is None else dev(torch, np.array([prev], f32))
                got_e = fm.expose(hist, prev=p, **meter)
                torch.cuda.synchronize()
                assert same(got_e.cpu().numpy(), np.array([want_e], f32)), (name, meter, prev, got_e, want_e)
                if p is not None:                             # in place: the state of a sequence
                    again = fm.expose(hist, prev=p, out=p, **meter)
                    torch.cuda.synchronize()
                    assert again.data_ptr() == p.data_ptr() and same(p.cpu().numpy(), np.array([want_e], f32)), (name, meter, prev)
    assert set(range(2040)) <= seen and 2047 in seen and not seen & set(range(2040, 2047))


def test_expose_on_handmade_histograms(torch, fm):
    """Histograms no frame gives: the rank in the first and the last slot a lane owns, on both sides of a lane's eight slots, counts
    whose sum passes 2^32, and a count in slot 2046, which holds no float."""
    cases = []
    for s in (1, 7, 8, 9, 15, 16, 1023, 1024, 2039, 2040, 2046):
        h = np.zeros(R.SLOTS, np.int64)
        h[0], h[2047], h[s] = 99, 99, 3
        cases.append(h)
    for a, b in ((7, 8), (8, 15), (15, 16), (1000, 1001), (1, 2046)):
        h = np.zeros(R.SLOTS, np.int64)
        h[a], h[b] = 10, 10
        cases.append(h)
    big = np.zeros(R.SLOTS, np.int64)
    big[900], big[1100], big[1101] = 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1
    cases.append(big)
    full = np.arange(R.SLOTS, dtype=np.int64) % 5
    cases.append(full)
    for i, h in enumerate(cases):
        hist = dev(torch, h.astype(np.uint32).view(np.int32))
        for meter in (dict(permille=1), dict(permille=500), dict(permille=501), dict(permille=666), dict(permille=667), dict(permille=1000),
                      dict(e_min=1e-38, e_max=3e38, rate=0.5)):
            for prev in (None, 1.5):
                want = R.expose(h, prev, **meter)
                got = fm.expose(hist, prev=None if prev is None else dev(torch, np.array([prev], f32)), **meter)
                torch.cuda.synchronize()
                assert same(got.cpu().numpy(), np.array([want], f32)), (i, meter, prev, got, want)


# ---- the drivers ----
def room_frames(sqt, torch, scene, n_frames, spp=4):
    cams = [sqt.camera_from_text(t) for t in TR.CAMERA_TEXTS[:n_frames]]
    return [scene.render_rows(cam, spp, TR.W, TR.H, want_rgb=False)[0] for cam in cams]


def test_film_auto_over_three_room_frames(sqt, torch, fm, O, scene):
    """Film(auto=...) over three frames of the room under a moving camera, each scaled differently so that the exposure has something
    to follow: bytes and state equal the restated chain; reset() starts over; a state set by hand is the chain's from there."""
    frames = [f * s for f, s in zip(room_frames(sqt, torch, scene, 3), (1.0, 6.0, 0.125))]
    torch.cuda.synchronize()
    host = [f.cpu().numpy() for f in frames]
    auto = dict(key=0.18, permille=500, rate=0.5)
    spec = dict(curve="reinhard", white=4.0, lut=fm.srgb_lut(256), dither=True)
    want = R.chain(O, host, spec, auto)
    exposures = [float(e) for _, e in want]
    assert len(set(exposures)) == 3 and exposures[1] < exposures[0]        # the brighter frame pulls the exposure down, half way
    film = sqt.Film(auto=auto, **spec)
    assert film.exposure_state is None
    for i, f in enumerate(frames):
        got = film(f)
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want[i][0]), i
        assert film.exposure_state == exposures[i]
    film.reset()
    assert film.exposure_state is None and np.array_equal(film.film(frames[0]).cpu().numpy(), want[0][0])
    film.exposure_state = exposures[0]                      # a checkpoint after frame 0, restored into the running film
    assert np.array_equal(film(frames[1]).cpu().numpy(), want[1][0]) and film.exposure_state == exposures[1]
    fresh = sqt.Film(auto=auto, **spec)                     # ... and into a new one, before its first frame
    assert fresh.prepare(0) is fresh and fresh._luts[torch.device("cuda", 0)].is_cuda      # the table is up before any frame
    assert sqt.Film().prepare(0)._luts == {}                # nothing to prepare without a table
    fresh.exposure_state = exposures[1]
    assert fresh.exposure_state == exposures[1] and np.array_equal(fresh(frames[2]).cpu().numpy(), want[2][0])
    # a state that lives on another device than the frame is refused, not dropped; reset() clears it
    fresh._state = fresh._state.cpu()
    with pytest.raises(fm.N.SquiglyError, match="reset\\(\\) it"):
        fresh(frames[2])
    fresh.reset()
    assert np.array_equal(fresh(frames[0]).cpu().numpy(), want[0][0])
    # without auto the exposure is the fixed one
    fixed = sqt.Film(curve="filmic", exposure=2.0)
    assert np.array_equal(fixed(frames[0]).cpu().numpy(), R.develop(O, host[0], 2.0, "filmic")[0]) and fixed.exposure_state is None


def test_temporal_and_sequence_take_a_film(sqt, torch, fm, O, product_scene, scene):
    """Temporal(film=): step's rgb is the film's image of step's avg, the other three results are what film=None gives, and
    render_sequence(film=) yields those images."""
    cams = [sqt.camera_from_text(t) for t in TR.CAMERA_TEXTS[:3]]
    spec = dict(curve="atan", lut=fm.gamma_lut(2.2, 64))
    auto = dict(rate=0.5)
    plain = sqt.Temporal(scene, TR.W, TR.H, 4)
    filmed = sqt.Temporal(scene, TR.W, TR.H, 4, film=sqt.Film(auto=auto, **spec))
    reference = sqt.Temporal(scene, TR.W, TR.H, 4, film=sqt.Film())
    avgs, images = [], []
    for cam in cams:
        a, b, c = plain.step(cam), filmed.step(cam), reference.step(cam)
        torch.cuda.synchronize()
        for x, y, z in zip(a[:3], b[:3], c[:3]):              # avg, var, length: the film touches none of them
            x, y, z = x.cpu().numpy(), y.cpu().numpy(), z.cpu().numpy()
            assert (same(x, y) and same(x, z)) if x.dtype == f32 else (np.array_equal(x, y) and np.array_equal(x, z))
        avgs.append(b[0].cpu().numpy())
        images.append(b[3].cpu().numpy())
        assert np.array_equal(c[3].cpu().numpy(), R.develop(O, avgs[-1])[0])
    want = R.chain(O, avgs, spec, auto)
    for i in range(3):
        assert np.array_equal(images[i], want[i][0]), i
    seq = list(sqt.render_sequence(product_scene[0], cams, 4, (TR.W, TR.H), film=sqt.Film(auto=auto, **spec)))
    assert len(seq) == 3 and all(np.array_equal(s, i) for s, i in zip(seq, images))


def test_render_adaptive_with_the_default_film_yields_todays_images(sqt, torch, product_scene):
    """render_adaptive(denoise=True, film=Film()) -- both variants -- yields bit for bit what film=None yields, tuple by tuple; another
    curve changes the last image only."""
    bih, cam, _ = product_scene
    for extra in (dict(), dict(lens=sqt.Lens(), subrays=4)):
        args = (bih, cam, 16, (TR.W, TR.H), 0.05)
        kw = dict(first=8, step=8, denoise=True, **extra)
        today = list(sqt.render_adaptive(*args, **kw))
        with_film = list(sqt.render_adaptive(*args, film=sqt.Film(), **kw))
        filmic = list(sqt.render_adaptive(*args, film=sqt.Film(curve="filmic", exposure=0.5), **kw))
        assert len(today) == len(with_film) == len(filmic) >= 2
        for a, b, c in zip(today, with_film, filmic):
            assert a[:3] == b[:3] == c[:3] and np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4]) and np.array_equal(a[4], c[4])
        assert all(np.array_equal(a[3], c[3]) for a, c in zip(today[:-1], filmic[:-1])) and not np.array_equal(today[-1][3], filmic[-1][3])
        assert today[-1][3].dtype == np.uint8 and today[-1][3].any()


def read_png(path):
    """The (rows, cols, 3) uint8 image of a file written by the package's write_png: 8-bit RGB, one IDAT, filter 0 on every row."""
    import struct
    import zlib
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, {}
    while pos < len(data):
        (n,), tag = struct.unpack(">I", data[pos:pos + 4]), data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF
        chunks[tag] = chunks.get(tag, b"") + body
        pos += 12 + n
    cols, rows, depth, colour, _, _, interlace = struct.unpack(">IIBBBBB", chunks[b"IHDR"])
    assert (depth, colour, interlace) == (8, 2, 0)
    raw = np.frombuffer(zlib.decompress(chunks[b"IDAT"]), np.uint8).reshape(rows, 1 + 3 * cols)
    assert (raw[:, 0] == 0).all()
    return raw[:, 1:].reshape(rows, cols, 3).copy()


def test_cli_film(sqt, tmp_path, monkeypatch):
    """The files the CLI writes hold, byte for byte, the images of the library call its flags stand for: --sequence --temporal with
    --film, --sequence alone (every frame exposed on its own), and --adaptive --denoise with --film.  Each differs from the same
    command without --film, so a film that main() dropped would show."""
    cli = importlib.import_module("squigly-trace_amd.cli")
    seq = tmp_path / "move.cams"
    seq.write_text("".join(t.decode() for t in TR.CAMERA_TEXTS[:3]))
    monkeypatch.chdir(os.path.dirname(DATA))
    bih = sqt.BIH(sqt.Mesh.from_obj(os.path.join(DATA, "scene.obj"), DATA))
    size = ["-s", "4", "-d", f"{TR.W},{TR.H}"]
    probe = np.zeros((2, 3, 3), np.uint8)
    probe[1, 2] = (1, 2, 250)
    sqt.write_png(str(tmp_path / "probe.png"), probe)
    assert np.array_equal(read_png(str(tmp_path / "probe.png")), probe)

    def files(name, flags):
        out = tmp_path / name
        assert cli.main(flags + size + ["-p", str(out)]) == 0
        return cli.parse_args(flags + size), str(out)

    film_flags = ["--film", "filmic", "--srgb", "--dither", "--auto-exposure", "0.25"]
    for temporal in (True, False):
        mode = ["--sequence", str(seq)] + (["--temporal"] if temporal else [])
        a, out = files(f"seq{int(temporal)}.png", mode + film_flags)
        _, plain_out = files(f"plain{int(temporal)}.png", mode)
        film = cli.film_of(a)
        want = list(sqt.render_sequence(bih, a.sequence, 4, (TR.W, TR.H), temporal=temporal, film=film))
        # the exposure follows a sequence that accumulates, and is forgotten with the history where it does not
        assert (film.exposure_state is not None) == temporal
        got = [read_png(p) for p in cli.view_paths(out, 3)]
        plain = [read_png(p) for p in cli.view_paths(plain_out, 3)]
        assert len(want) == 3
        for i in range(3):
            assert np.array_equal(got[i], want[i]), (temporal, i)
            assert got[i].any() and not np.array_equal(got[i], plain[i]), (temporal, i)
    adaptive = ["--adaptive", "0.05", "--denoise"]
    a, out = files("adaptive.png", adaptive + ["--film", "reinhard", "--white", "3", "--exposure", "0.5"])
    _, plain_out = files("adaptive_plain.png", adaptive)
    cam = sqt.load_camera(os.path.join(DATA, "camera"))
    kw = dict(eps=a.adaptive_eps, first=a.adaptive_first, step=a.adaptive_step, denoise=a.denoise)
    want = list(sqt.render_adaptive(bih, cam, 4, (TR.W, TR.H), a.adaptive, film=cli.film_of(a), **kw))[-1][3]
    today = list(sqt.render_adaptive(bih, cam, 4, (TR.W, TR.H), a.adaptive, **kw))[-1][3]
    assert np.array_equal(read_png(out), want) and np.array_equal(read_png(plain_out), today) and not np.array_equal(want, today) and want.any()
