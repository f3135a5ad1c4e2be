"""The temporal accumulation without a GPU: the library's surface (exports, ids, refusals, block size), its host-side projection
against the numpy restatement and under the sanitizers, and what the specified accumulation -- the restatement -- does on the
two-plane synthetic frames and on the project's own scene rendered by the oracle."""
import ctypes as C
import importlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import denoise_restatement as DR
import library_surface as LS
import temporal_restatement as R
import temporal_room as TR
from bitcmp import bits, same
from denoise_room import room

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NO_DEVICE = 1 << 20         # a device number no machine has: a call the checks let through by mistake fails there, before any launch


@pytest.fixture(scope="module")
def tp(sqt):
    mod = importlib.import_module("squigly-trace_amd.temporal")
    mod.lib()
    return mod


def test_header_functions_are_exported(tp):
    declared = LS.check_exports(tp, "squigly_temporal.h", "sq_temporal_")    # (and nothing of another library's leaks out of this one)
    assert {"sq_temporal_accumulate_device", "sq_temporal_unpack_device", "sq_temporal_project", "sq_temporal_history_bytes"} <= declared
    # not a client of the main library: it reads its header for sq_camera and calls nothing of it
    LS.check_client(tp.LIB_PATH, False)


def test_six_ids_are_distinct_and_an_edit_moves_only_its_own(tp, sqt, tmp_path):
    b = LS.build_module()                                     # (six when this library landed; the table has grown since)
    assert len(b.LIBS) >= 6
    assert "sq_temporal.hip" not in LS.files(b, "main")
    assert "sq_temporal_pixel.h" not in b.LIBS["main"]["headers"] + b.LIBS["denoise"]["headers"] + b.LIBS["shutter"]["headers"]
    t = b.LIBS["temporal"]
    assert t["salt"] == b"temporal\0" and t["macro"] == "SQ_TEMPORAL_BUILD_ID" and t["link"] == []
    LS.check_ids(b, "temporal", tp, sqt, tmp_path, [("sq_temporal.hip", {"temporal"}), ("sq_temporal_pixel.h", {"temporal"})])


def test_history_bytes_is_monotone(tp):
    hb = tp.history_bytes
    sizes = [1, 2, 3, 15, 16, 17, 63, 64, 65, 255, 1080, 1920, 4096, 46340]
    for r in sizes:
        for c0, c1 in zip(sizes, sizes[1:]):
            assert 0 < hb(r, c0) <= hb(r, c1) and hb(c0, r) <= hb(c1, r)
    assert hb(1920, 1080) == hb(1080, 1920) == 1920 * 1080 * 48 and hb(1, 1) == 48
    assert hb(0, 5) == hb(5, 0) == hb(-1, 5) == hb(5, -2) == 0
    assert hb(2 ** 31 - 1, 1) > 0 and hb(46341, 46341) == 0 and hb(2 ** 31 - 1, 2) == 0


# ---- refusals: nothing here reaches a device, the pointers are numbers that are never followed ----
BUF = {name: 0x10000000 + i * 0x100000 for i, name in enumerate(("color", "var", "tri", "normal", "point", "alpha", "prev", "next", "out",
                                                                  "out_var", "out_len"))}
BLOCK = 6 * 5 * 48


def call(tp, sqt, rows=6, cols=5, params=None, null_params=False, null_cam=False, **ptr):
    p = dict(alpha_min=0.1, max_history=32, sigma_p=0.05, cos_n=0.9)
    p.update(params or {})
    P = tp.Params(p["alpha_min"], p["max_history"], p["sigma_p"], p["cos_n"])
    a = {**BUF, **ptr}
    cam = sqt.Camera()
    rc = tp.lib().sq_temporal_accumulate_device(NO_DEVICE, rows, cols, a["color"], a["var"], a["tri"], a["normal"], a["point"], a["alpha"],
                                                None if null_cam else C.byref(cam), a["prev"], None if null_params else C.byref(P),
                                                a["next"], a["out"], a["out_var"], a["out_len"], None)
    return rc, tp.lib().sq_temporal_last_error().decode()


nan = float("nan")
REFUSALS = [
    (dict(color=None), "null argument"), (dict(var=None), "null argument"), (dict(tri=None), "null argument"),
    (dict(normal=None), "null argument"), (dict(point=None), "null argument"), (dict(next=None), "null argument"),
    (dict(out=None), "null argument"), (dict(out_var=None), "null argument"), (dict(null_params=True), "null argument"),
    (dict(null_cam=True), "prev_cam is required"),
    (dict(rows=0), "at least 1"), (dict(cols=0), "at least 1"), (dict(rows=-3), "at least 1"),
    (dict(rows=46341, cols=46341), "exceed 2\\^31 - 1"),
    (dict(params={"alpha_min": -0.01}), "alpha_min"), (dict(params={"alpha_min": 1.01}), "alpha_min"), (dict(params={"alpha_min": nan}), "alpha_min"),
    (dict(params={"max_history": 0}), "max_history"), (dict(params={"max_history": 65537}), "max_history"), (dict(params={"max_history": -1}), "max_history"),
    (dict(params={"sigma_p": -1e-3}), "sigma_p"), (dict(params={"sigma_p": nan}), "sigma_p"),
    (dict(params={"cos_n": nan}), "cos_n"),
    (dict(prev=BUF["prev"] + 4), "d_prev must be 16-byte aligned"), (dict(next=BUF["next"] + 8), "d_next must be 16-byte aligned"),
    (dict(next=BUF["prev"]), "d_prev and d_next overlap"), (dict(next=BUF["prev"] + BLOCK - 16), "d_prev and d_next overlap"),
    (dict(out=BUF["color"] + 12), "d_color and d_out overlap"),                 # shifted by a pixel: not the allowed d_out == d_color
    (dict(out_var=BUF["var"] + 4), "d_var and d_out_var overlap"),
    (dict(out=BUF["normal"]), "d_normal and d_out overlap"), (dict(out=BUF["point"]), "d_point and d_out overlap"),
    (dict(out=BUF["tri"]), "d_tri and d_out overlap"), (dict(out_var=BUF["color"]), "d_color and d_out_var overlap"),
    (dict(out_len=BUF["tri"]), "d_tri and d_out_len overlap"), (dict(out_len=BUF["var"]), "d_var and d_out_len overlap"),
    (dict(alpha=BUF["var"]), "d_var and d_alpha overlap"), (dict(out_var=BUF["alpha"]), "d_alpha and d_out_var overlap"),
    (dict(color=BUF["normal"]), "d_color and d_normal overlap"),
    (dict(out=BUF["next"] + 16), "d_next and d_out overlap"), (dict(color=BUF["prev"] + BLOCK - 16), "d_color and d_prev overlap"),
    (dict(next=BUF["color"] - BLOCK + 16), "d_color and d_next overlap"),
    (dict(out=BUF["out_var"] - 4), "d_out and d_out_var overlap"), (dict(out_len=BUF["out"]), "d_out and d_out_len overlap"),
]


@pytest.mark.parametrize("kw, message", REFUSALS, ids=[f"{i:02d}-{m[:12]}" for i, (_, m) in enumerate(REFUSALS)])
def test_refusals_need_no_gpu(tp, sqt, kw, message):
    rc, err = call(tp, sqt, **kw)
    assert rc != 0 and re.search(message, err), err


def test_what_is_allowed_gets_past_the_checks(tp, sqt):
    """d_out == d_color, d_out_var == d_var, a call without history (and then without a camera), without d_alpha and without
    d_out_len, and the extreme parameters pass every check: on a device that does not exist they fail at the first runtime call,
    and with its message."""
    for kw in (dict(), dict(out=BUF["color"]), dict(out_var=BUF["var"]), dict(out=BUF["color"], out_var=BUF["var"]),
               dict(prev=None), dict(prev=None, null_cam=True), dict(alpha=None), dict(out_len=None),
               dict(params={"alpha_min": 0.0, "max_history": 1, "sigma_p": 0.0, "cos_n": -float("inf")}),
               dict(params={"alpha_min": 1.0, "max_history": 65536, "sigma_p": float("inf"), "cos_n": 2.0})):
        rc, err = call(tp, sqt, **kw)
        assert rc != 0 and "hipSetDevice" in err, (kw, err)


def test_unpack_refusals(tp):
    L = tp.lib()
    h, outs = 0x1000000, [0x2000000 + i * 0x100000 for i in range(6)]
    cases = [((6, 5, None, *outs), "d_hist is required"), ((6, 5, h, *[None] * 6), "no output"), ((0, 5, h, *outs), "at least 1"),
             ((46341, 46341, h, *outs), "exceed"), ((6, 5, h + 4, *outs), "16-byte aligned"),
             ((6, 5, h, h + 16, *outs[1:]), "d_hist and d_color overlap"), ((6, 5, h, outs[0], outs[0], *outs[2:]), "d_color and d_var overlap"),
             ((6, 5, h, *outs[:5], outs[3]), "d_tri and d_point overlap")]
    for args, message in cases:
        assert L.sq_temporal_unpack_device(NO_DEVICE, *args, None) != 0
        assert message in L.sq_temporal_last_error().decode(), (message, L.sq_temporal_last_error().decode())
    for args in ((6, 5, h, *outs), (6, 5, h, None, None, outs[2], None, None, None)):
        assert L.sq_temporal_unpack_device(NO_DEVICE, *args, None) != 0 and "hipSetDevice" in L.sq_temporal_last_error().decode()


def test_python_refusals(tp, sqt):
    with pytest.raises(tp.N.SquiglyError, match="sigma_p is required"):
        tp.make_params()
    with pytest.raises(tp.N.SquiglyError, match="unknown temporal parameter"):
        tp.make_params(sigma_p=0.1, sigma=3)
    with pytest.raises(tp.N.SquiglyError, match="max_history must be an integer"):
        tp.make_params(sigma_p=0.1, max_history=2.0)
    p = tp.make_params(sigma_p=0.25, max_history=7)
    assert (p.max_history, p.sigma_p, p.alpha_min, p.cos_n) == (7, 0.25, f32(0.1), f32(0.9))
    cam = sqt.Camera()
    for bad in ((cam, 0, 5, (1, 2, 3)), (cam, 5, -1, (1, 2, 3))):
        with pytest.raises(tp.N.SquiglyError, match="at least 1"):
            tp.project(*bad)
    pt, out = (C.c_float * 3)(), C.c_float()
    assert tp.lib().sq_temporal_project(None, 4, 4, pt, C.byref(out), C.byref(out)) < 0
    assert tp.lib().sq_temporal_project(C.byref(cam), 4, 4, pt, None, C.byref(out)) < 0
    assert "null argument" in tp.lib().sq_temporal_last_error().decode()


def test_temporal_argument_refusals(sqt):
    """Temporal refuses its numbers before it looks at the scene (None here)."""
    for kw, message in ((dict(spp=0), "spp"), (dict(spp=2.0), "spp"), (dict(spp=True), "spp"), (dict(period=0), "period"),
                        (dict(spp=2 ** 20, period=2 ** 12), "exceed"), (dict(max_history=0), "max_history"),
                        (dict(max_history=65537), "max_history"), (dict(alpha_min=-0.1), "alpha_min"), (dict(alpha_min=1.5), "alpha_min"),
                        (dict(alpha_min=float("nan")), "alpha_min"), (dict(alpha_min="0.1"), "alpha_min"), (dict(frames=-1), "frames"),
                        (dict(history=np.zeros(8, np.uint8)), "resuming needs"), (dict(camera=sqt.Camera()), "resuming needs")):
        args = dict(spp=16)
        args.update(kw)
        spp = args.pop("spp")
        with pytest.raises(ValueError, match=message):
            sqt.Temporal(None, 48, 64, spp, **args)
    render = importlib.import_module("squigly-trace_amd.render")
    with pytest.raises(ValueError, match="at least one camera"):
        next(render.render_sequence(None, [], 16, (48, 64)))
    with pytest.raises(ValueError, match="spp"):
        next(render.render_sequence(None, [sqt.Camera()], 0, (48, 64)))
    with pytest.raises(ValueError, match="denoise must be"):
        next(render.render_sequence(None, [sqt.Camera()], 4, (48, 64), denoise=-1.0))


def test_cli_sequence_flags(sqt, tmp_path):
    cli = importlib.import_module("squigly-trace_amd.cli")
    seq = tmp_path / "move.cams"
    seq.write_text("".join(t.decode() for t in TR.CAMERA_TEXTS[:3]))
    a = cli.parse_args(["--sequence", str(seq), "--temporal"])
    assert a.temporal is True and len(a.sequence) == 3 and a.denoise is None
    assert bytes(a.sequence[1]) == bytes(sqt.camera_from_text(TR.CAMERA_TEXTS[1]))
    assert cli.parse_args(["--sequence", str(seq), "--temporal", "0.25", "--denoise"]).temporal == 0.25
    assert cli.parse_args(["--sequence", str(seq), "--temporal", "1"]).temporal == 1.0
    assert cli.parse_args(["--sequence", str(seq)]).temporal is None                      # plain frames of the same samples
    assert cli.parse_args([]).sequence is None
    assert cli.view_paths("out/move.png", 2) == ["out/move_0000.png", "out/move_0001.png"]
    odd = tmp_path / "odd.cams"
    odd.write_text("0 7 0.75\n")
    for bad in (["--temporal"], ["--temporal", "0.2"], ["--sequence", str(seq), "--temporal", "--adaptive", "0.5"],
                ["--sequence", str(seq), "--temporal", "--aa"], ["--sequence", str(seq), "--temporal", "--aa", "0.5"],
                ["--sequence", str(seq), "--temporal", "1.5"], ["--sequence", str(seq), "--temporal", "nan"],
                ["--sequence", str(seq), "--cast"], ["--sequence", str(seq), "--views", str(seq)], ["--sequence", str(seq), "--aperture", "0.1"],
                ["--sequence", str(odd)], ["--sequence", str(tmp_path / "missing")]):
        with pytest.raises(SystemExit):
            cli.parse_args(bad)


# ---- the projection ----
def product_cam(sqt, text):
    return sqt.camera_from_text(text)


def room_points(O, oracle_scene):
    rm = room(O, oracle_scene)
    hit = rm["tri"] >= 0
    return rm, hit


def test_project_is_the_restatement_on_the_rooms_points(tp, sqt, O, oracle_scene, tmp_path):
    """sq_temporal_project against the restatement, bit for bit, for the room's first hits under the frame's own camera and under a
    camera of the sequence, and for points behind the camera, outside the image and not numbers; then tests/temporal_main.cpp (its own
    main over csrc/sq_temporal_pixel.h, the text the library compiles) built with -fsanitize=address,undefined and run once over the
    same points: exit 0, nothing on stderr, the same bits."""
    rm, hit = room_points(O, oracle_scene)
    inf = float("inf")
    extra = np.array([[0, 9, 0.75], [0, 7, 0.75], [40, 0, 0], [0, 0, 90], [nan, 0, 0], [0, inf, 0], [0, -inf, 0], [1e30, -1e30, 1e30]], f32)
    points = np.concatenate([rm["point"][hit], extra])
    exe = str(tmp_path / "temporal_main")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-static-libasan", "-static-libubsan",      # the runtimes inside the program: nothing to order at load time
                           os.path.join(ROOT, "tests", "temporal_main.cpp"), "-o", exe], stderr=subprocess.DEVNULL)
    seen = set()
    for text in (open(os.path.join(ROOT, "data", "camera"), "rb").read(), TR.CAMERA_TEXTS[0]):
        cam = product_cam(sqt, text)
        ok, fx, fy = R.project(cam, TR.W, TR.H, points)
        seen |= set(ok.tolist())
        got = [tp.project(cam, TR.W, TR.H, p) for p in points]
        words = ["%08x" % int(u) for u in bits(np.array(list(cam.pos) + list(cam.rot), f32)).view(np.uint32)]
        words += ["%08x" % int(u) for u in bits(points).view(np.uint32).reshape(-1)]
        r = subprocess.run([exe, str(TR.W), str(TR.H)] + words, capture_output=True)
        assert r.returncode == 0 and r.stderr == b"", (r.returncode, r.stderr[-2000:])
        lines = r.stdout.decode().splitlines()
        assert len(lines) == len(points)
        for i, (line, (g_ok, g_fx, g_fy)) in enumerate(zip(lines, got)):
            m_ok, m_fx, m_fy = line.split()
            assert g_ok == bool(ok[i]) == (m_ok == "1"), (i, points[i])
            if ok[i]:          # (fx and fy of a point that does not project are not meaningful)
                want = (int(bits(fx[i:i + 1]).view(np.uint32)[0]), int(bits(fy[i:i + 1]).view(np.uint32)[0]))
                assert (int(m_fx, 16), int(m_fy, 16)) == want, (i, points[i])
                assert (int(bits(np.array([g_fx], f32)).view(np.uint32)[0]), int(bits(np.array([g_fy], f32)).view(np.uint32)[0])) == want
        assert not ok[-len(extra):][[0, 4, 5, 6]].any()                # behind the camera, NaN, infinite
    assert seen == {True, False}


def test_round_trip_on_the_room(O, oracle_scene):
    """With prev == cam every hit pixel of the oracle's 48 x 64 room projects to its own (column, row) within 1/64 pixel.  (Measured:
    3.8e-6 pixel at most, in both coordinates -- the rounding of the oracle's hit point, not of the projection.)"""
    rm, hit = room_points(O, oracle_scene)
    assert hit.sum() > 1000
    ok, fx, fy = R.project(oracle_scene[1], TR.W, TR.H, rm["point"])
    yy, xx = np.mgrid[0:TR.W, 0:TR.H]
    assert ok[hit].all()
    ex, ey = np.abs(fx.astype(np.float64) - xx)[hit].max(), np.abs(fy.astype(np.float64) - yy)[hit].max()
    print(f"round trip: max |fx - x| = {ex:.3g}, max |fy - y| = {ey:.3g}")
    assert ex <= 1 / 64 and ey <= 1 / 64


# ---- the restatement itself ----
def test_restatement_edges():
    cam = ((0, 0, 0), R.IDENTITY)
    frame = R.synthetic(17, 23, seed=3, cam=cam)
    color, var, tri = frame[:3]
    assert (tri < 0).any() and (tri == R.FAR_TRI).any() and (tri == R.NEAR_TRI).any()
    assert np.isnan(color).any() and np.isinf(color).any() and (var == 0).any()
    first = R.accumulate(*frame, None, None)
    assert same(first["color"], color) and same(first["var"], var) and (first["len"] == 1).all()
    assert all(k in first["block"] for k in R.BLOCK_FIELDS) and np.array_equal(first["block"]["tri"], tri)
    # the same frame again under the same camera: every hit pixel finds itself, or a neighbour of its own plane
    again = R.accumulate(*frame, cam, first["block"], sigma_p=0.05)
    hit = tri >= 0
    assert (again["len"][hit] == 2).all() and (again["len"][~hit] == 1).all()
    assert same(again["color"][~hit], color[~hit]) and same(again["var"][~hit], var[~hit])
    assert not same(again["color"][hit], color[hit])
    # max_history stops the length; alpha_min = 1 and alpha = 1 are the same weight, and the length goes on counting under it
    third = R.accumulate(*frame, cam, again["block"], sigma_p=0.05, max_history=2)
    assert (third["len"][hit] == 2).all()
    keep = R.accumulate(*frame, cam, again["block"], sigma_p=0.05, alpha_min=1.0)
    ones = R.accumulate(*frame, cam, again["block"], sigma_p=0.05, alpha=np.ones(tri.shape, f32))
    assert same(keep["color"], ones["color"]) and same(keep["var"], ones["var"]) and (keep["len"][hit] == 3).all()
    finite = hit & np.isfinite(keep["color"]).all(-1)
    assert finite.sum() > 50 and np.allclose(keep["color"][finite], color[finite], rtol=1e-5, atol=1e-6)
    # a previous frame that is all background, and one seen from behind, give no history
    empty = dict(first["block"], tri=np.full(tri.shape, -1, np.int32))
    assert (R.accumulate(*frame, cam, empty)["len"] == 1).all()
    assert (R.accumulate(*frame, ((10, 0, 0), R.IDENTITY), first["block"])["len"] == 1).all()


def test_disocclusion_on_the_two_planes():
    """A sideways camera step over the two-plane frame: the strip in front moves across the wall.  A wall pixel all of whose taps in
    the previous frame are strip pixels is newly revealed -- len 1 and its input colour bit for bit; a wall pixel whose four taps are
    wall pixels keeps len 2; and a pixel between the two takes the wall taps it has."""
    rows, cols = 48, 64
    cam0, cam1 = ((0, 0, 0), R.IDENTITY), ((0, 0.4, 0), R.IDENTITY)
    f0, f1 = R.synthetic(rows, cols, 5, cam0), R.synthetic(rows, cols, 6, cam1)
    b0 = R.first_block(*f0)
    out = R.accumulate(*f1, cam0, b0, sigma_p=0.05)
    tri1, tri0 = f1[2], f0[2]
    ok, fx, fy = R.project(cam0, rows, cols, f1[4])
    x0, y0 = np.floor(np.where(ok, fx, 0)).astype(int), np.floor(np.where(ok, fy, 0)).astype(int)
    strip = np.zeros((rows, cols), int)
    wall = np.zeros((rows, cols), int)
    for j in (0, 1):
        for i in (0, 1):
            qy, qx = y0 + j, x0 + i
            inside = ok & (qy >= 0) & (qy < rows) & (qx >= 0) & (qx < cols)
            t = np.where(inside, tri0[np.clip(qy, 0, rows - 1), np.clip(qx, 0, cols - 1)], -1)
            strip += t == R.NEAR_TRI
            wall += t == R.FAR_TRI
    far = tri1 == R.FAR_TRI
    revealed, kept, between = far & (strip == 4), far & (wall == 4), far & (strip > 0) & (wall > 0)
    assert revealed.sum() >= 20 and kept.sum() >= 500 and between.sum() >= 10
    assert (out["len"][revealed] == 1).all()
    assert same(out["color"][revealed], f1[0][revealed]) and same(out["var"][revealed], f1[1][revealed])
    assert (out["len"][kept] == 2).all()
    assert (out["len"][between] == 2).all()
    near = tri1 == R.NEAR_TRI
    assert (out["len"][near & (strip == 4)] == 2).all() and (out["len"][tri1 < 0] == 1).all()


QUALITY_RATIO = 0.1343       # measured with the restatement and the oracle when the contract was written


def test_quality_on_the_room_sequence(O, oracle_scene):
    """Eight frames of the room at 48 x 64 and 16 spp under a camera that steps 0.04 along x a frame; frame f is the slice
    [16 f, 16 f + 16) of the oracle's 128-sample frame of its camera.  Demodulated, alpha from `reflective`, default parameters, no
    spatial filter.  The mean squared error of the eighth accumulated frame against the oracle's 1024-spp frame of the eighth camera,
    over the hit pixels, as a ratio to the eighth noisy frame's: measured 0.1343 (noisy 1.4135, accumulated 0.1898); asserted at most
    1.25 x that.  More than half of the hit pixels end with len >= 4 (measured: 98 %) and some with len 1 (measured: 21), so the
    sequence does reproject and does disocclude."""
    seq = TR.sequence(O, oracle_scene)
    frames, alphas, demod = [], [], []
    counts = np.full((TR.W, TR.H), TR.SPP, np.int32)
    for fr in seq["frames"]:
        g = fr["guides"]
        x, v, ok, scale = TR.demodulate(fr["avg"], DR.variance(fr["sums"], fr["sums2"], counts), g)
        frames.append((x, v, g["tri"], g["normal"], g["point"]))
        alphas.append(g["reflective"])
        demod.append((g, ok, scale))
    outs = R.chain(frames, seq["cams"], alphas, **R.DEFAULTS)
    last = outs[-1]
    out, out_var = TR.remodulate(last["color"], last["var"], *demod[-1])
    hit = seq["frames"][-1]["guides"]["tri"] >= 0
    assert 0.3 < hit.mean() < 1.0
    ref = seq["ref"].astype(np.float64)
    mse = lambda img: ((img.astype(np.float64) - ref)[hit] ** 2).mean()  # noqa: E731
    noisy, acc = mse(seq["frames"][-1]["avg"]), mse(out)
    print(f"noisy mse {noisy:.4f}; accumulated mse {acc:.4f}; ratio {acc / noisy:.4f}")
    assert acc / noisy <= 1.25 * QUALITY_RATIO, (noisy, acc)
    length = last["len"][hit]
    assert (length >= 4).mean() > 0.5 and (length == 1).sum() >= 1 and length.max() == TR.FRAMES
    assert np.isfinite(out_var[hit]).all() and (out_var[hit] >= 0).all()
