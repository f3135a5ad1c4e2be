"""The display stage without a GPU: the library's surface (exports, ids, refusals), the Python layer's and the command line's
refusals, and the specified arithmetic -- the numpy restatement -- held against tests/film_main.cpp, a host program over
csrc/sq_film_pixel.h (the text the kernels compile), built plainly and under the sanitizers."""
import ctypes as C
import importlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import film_restatement as R
import library_surface as LS
from bitcmp import same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NO_DEVICE = 1 << 20         # a device number no machine has: a call the checks let through by mistake fails there, before any launch
nan, inf = float("nan"), float("inf")


@pytest.fixture(scope="module")
def fm(sqt):
    mod = importlib.import_module("squigly-trace_amd.film")
    mod.lib()
    return mod


def test_header_functions_are_exported(fm):
    declared = LS.check_exports(fm, "squigly_film.h", "sq_film_")            # (and nothing of another library's leaks out of this one)
    assert {"sq_film_histogram_device", "sq_film_expose_device", "sq_film_develop_device", "sq_film_build_id", "sq_film_last_error"} == declared
    LS.check_client(fm.LIB_PATH, False)                        # not a client of the main library


def test_seven_ids_are_distinct_and_an_edit_moves_only_the_films(fm, sqt, tmp_path):
    b = LS.build_module()
    assert list(b.LIBS) == ["denoise", "main", "lens", "mlens", "shutter", "temporal", "film"]     # seven, in the order they are built
    others = LS.files(b, "main") + b.LIBS["denoise"]["headers"] + b.LIBS["shutter"]["headers"] + b.LIBS["temporal"]["headers"]
    assert "sq_film.hip" not in others and "sq_film_pixel.h" not in others and "../../include/squigly_film.h" not in others
    film = b.LIBS["film"]
    assert film["salt"] == b"film\0" and film["macro"] == "SQ_FILM_BUILD_ID" and film["link"] == []
    after = LS.check_ids(b, "film", fm, sqt, tmp_path, [("sq_film.hip", {"film"}), ("sq_film_pixel.h", {"film"})])
    # a variant build (tools/gpu_film.py's folding forms) has an id of its own
    assert b.lib_source_id(film, ["-DSQ_FILM_HIST_FOLD=0"]) != after["film"]


# ---- refusals: nothing here reaches a device, the pointers are numbers that are never followed ----
BUF = {name: 0x10000000 + i * 0x100000 for i, name in enumerate(("color", "hist", "prev", "exposure", "lut", "rgb", "display"))}
ROWS, COLS = 6, 5
N = ROWS * COLS


def last(fm):
    return fm.lib().sq_film_last_error().decode()


def call_histogram(fm, rows=ROWS, cols=COLS, **ptr):
    a = {**BUF, **ptr}
    return fm.lib().sq_film_histogram_device(NO_DEVICE, rows, cols, a["color"], a["hist"], None), last(fm)


def call_expose(fm, meter=None, null_meter=False, **ptr):
    a = {**BUF, **ptr}
    m = dict(R.METER, **(meter or {}))
    M = fm.Meter(m["key"], m["permille"], m["e_min"], m["e_max"], m["rate"], m["fallback"])
    return fm.lib().sq_film_expose_device(NO_DEVICE, a["hist"], None if null_meter else C.byref(M), a["prev"], a["exposure"], None), last(fm)


def call_develop(fm, rows=ROWS, cols=COLS, params=None, null_params=False, **ptr):
    a = {**BUF, "lut": None, **ptr}
    p = dict(exposure=1.0, curve=1, white=inf, n_lut=0, dither=0)
    p.update(params or {})
    P = fm.Params(p["exposure"], p["curve"], p["white"], p["n_lut"], p["dither"])
    return fm.lib().sq_film_develop_device(NO_DEVICE, rows, cols, a["color"], a["exposure"], None if null_params else C.byref(P), a["lut"],
                                           a["rgb"], a["display"], None), last(fm)


SIZES = [(dict(rows=0), "at least 1"), (dict(cols=0), "at least 1"), (dict(rows=-3), "at least 1"), (dict(rows=46341, cols=46341), "exceed 2\\^31 - 1")]
HISTOGRAM_REFUSALS = SIZES + [
    (dict(color=None), "null argument"), (dict(hist=None), "null argument"),
    (dict(hist=BUF["hist"] + 2), "d_hist must be 4-byte aligned"), (dict(hist=BUF["hist"] + 1), "4-byte aligned"),
    (dict(hist=BUF["color"]), "d_color and d_hist overlap"), (dict(hist=BUF["color"] + 12 * N - 4), "d_color and d_hist overlap"),
    (dict(color=BUF["hist"] + 8188), "d_color and d_hist overlap"),
]
EXPOSE_REFUSALS = [
    (dict(hist=None), "null argument"), (dict(exposure=None), "null argument"), (dict(null_meter=True), "null argument"),
    (dict(hist=BUF["hist"] + 2), "d_hist must be 4-byte aligned"),
    (dict(meter={"permille": 0}), "permille"), (dict(meter={"permille": 1001}), "permille"), (dict(meter={"permille": -5}), "permille"),
    (dict(meter={"e_min": 0.0}), "e_min"), (dict(meter={"e_min": -1.0}), "e_min"), (dict(meter={"e_min": nan}), "e_min"),
    (dict(meter={"e_max": inf}), "e_max"), (dict(meter={"e_max": nan}), "e_max"), (dict(meter={"e_min": 2.0, "e_max": 1.0}), "e_min <= e_max"),
    (dict(meter={"rate": -0.1}), "rate"), (dict(meter={"rate": 1.5}), "rate"), (dict(meter={"rate": nan}), "rate"),
    (dict(meter={"fallback": 0.0}), "fallback"), (dict(meter={"fallback": -1.0}), "fallback"), (dict(meter={"fallback": nan}), "fallback"),
    (dict(prev=BUF["hist"] + 16), "d_hist and d_prev overlap"), (dict(exposure=BUF["hist"] + 8188), "d_hist and d_exposure overlap"),
    (dict(prev=BUF["exposure"] + 2), "d_prev and d_exposure overlap"),                     # shifted: not the allowed d_prev == d_exposure
]
DEVELOP_REFUSALS = SIZES + [
    (dict(color=None), "null argument"), (dict(rgb=None), "null argument"), (dict(null_params=True), "null argument"),
    (dict(params={"curve": -1}), "curve"), (dict(params={"curve": 5}), "curve"),
    (dict(params={"curve": 2, "white": 0.0}), "white"), (dict(params={"curve": 2, "white": -1.0}), "white"), (dict(params={"curve": 2, "white": nan}), "white"),
    (dict(lut=BUF["lut"], params={"n_lut": 1}), "n_lut"), (dict(lut=BUF["lut"], params={"n_lut": 0}), "n_lut"),
    (dict(lut=BUF["lut"], params={"n_lut": 65537}), "n_lut"), (dict(lut=BUF["lut"], params={"n_lut": -4}), "n_lut"),
    (dict(params={"dither": 2}), "dither"), (dict(params={"dither": -1}), "dither"),
    (dict(params={"curve": 0, "dither": 1}), "reference curve"), (dict(lut=BUF["lut"], params={"curve": 0, "n_lut": 16}), "reference curve"),
    (dict(rgb=BUF["color"]), "d_color and d_rgb overlap"), (dict(rgb=BUF["color"] + 12 * N - 1), "d_color and d_rgb overlap"),
    (dict(display=BUF["color"]), "d_color and d_display overlap"),                         # not even in place
    (dict(display=BUF["rgb"] + 3 * N - 1), "d_rgb and d_display overlap"), (dict(rgb=BUF["display"] + 4), "d_rgb and d_display overlap"),
    (dict(exposure=BUF["color"] + 8), "d_color and d_exposure overlap"), (dict(exposure=BUF["rgb"]), "d_exposure and d_rgb overlap"),
    (dict(exposure=BUF["display"] + 12 * N - 4), "d_exposure and d_display overlap"),
    (dict(lut=BUF["color"], params={"n_lut": 2}), "d_color and d_lut overlap"), (dict(lut=BUF["rgb"] - 4, params={"n_lut": 2}), "d_lut and d_rgb overlap"),
    (dict(lut=BUF["display"], params={"n_lut": 2}), "d_lut and d_display overlap"), (dict(lut=BUF["exposure"], params={"n_lut": 2}), "d_exposure and d_lut overlap"),
]
ids_of = lambda cases: [f"{i:02d}-{m[:12]}" for i, (_, m) in enumerate(cases)]  # noqa: E731


@pytest.mark.parametrize("kw, message", HISTOGRAM_REFUSALS, ids=ids_of(HISTOGRAM_REFUSALS))
def test_histogram_refusals_need_no_gpu(fm, kw, message):
    rc, err = call_histogram(fm, **kw)
    assert rc != 0 and re.search(message, err), err


@pytest.mark.parametrize("kw, message", EXPOSE_REFUSALS, ids=ids_of(EXPOSE_REFUSALS))
def test_expose_refusals_need_no_gpu(fm, kw, message):
    rc, err = call_expose(fm, **kw)
    assert rc != 0 and re.search(message, err), err


@pytest.mark.parametrize("kw, message", DEVELOP_REFUSALS, ids=ids_of(DEVELOP_REFUSALS))
def test_develop_refusals_need_no_gpu(fm, kw, message):
    rc, err = call_develop(fm, **kw)
    assert rc != 0 and re.search(message, err), err


def test_what_is_allowed_gets_past_the_checks(fm):
    """Every optional pointer left out or given, d_prev == d_exposure, buffers that start anywhere, the extreme parameters and values
    that are merely odd pass every check: on a device that does not exist they fail at the first runtime call, with its message."""
    cases = [call_histogram(fm), call_histogram(fm, color=BUF["color"] + 4), call_histogram(fm, rows=2 ** 31 - 1, cols=1, hist=0x7000000000),
             call_expose(fm), call_expose(fm, prev=None), call_expose(fm, prev=BUF["exposure"]),
             call_expose(fm, meter={"permille": 1, "rate": 0.0, "e_min": 1e-38, "e_max": 3e38, "fallback": inf, "key": nan}),
             call_expose(fm, meter={"permille": 1000, "rate": 1.0, "e_min": 2.0, "e_max": 2.0, "key": -1.0}),
             call_develop(fm), call_develop(fm, exposure=None, display=None), call_develop(fm, color=BUF["color"] + 4, rgb=BUF["rgb"] + 1),
             call_develop(fm, params={"exposure": nan}), call_develop(fm, params={"exposure": -inf, "curve": 4, "dither": 1}),
             call_develop(fm, params={"curve": 0, "white": 0.0, "n_lut": 99}),                 # white and n_lut are not read here
             call_develop(fm, params={"curve": 2, "white": inf}), call_develop(fm, params={"curve": 2, "white": 1e-30, "dither": 1}),
             call_develop(fm, lut=BUF["lut"], params={"curve": 3, "n_lut": 2}), call_develop(fm, lut=BUF["lut"], params={"curve": 4, "n_lut": 65536, "dither": 1})]
    for i, (rc, err) in enumerate(cases):
        assert rc != 0 and "hipSetDevice" in err, (i, err)


def test_python_refusals(fm, sqt):
    E = fm.N.SquiglyError
    for kw, message in ((dict(speed=1), "unknown meter parameter"), (dict(permille=0), "permille"), (dict(permille=500.0), "permille"),
                        (dict(permille=True), "permille"), (dict(e_min=0), "e_min"), (dict(e_max=inf), "e_min and e_max"), (dict(e_min=3, e_max=2), "e_min"),
                        (dict(rate=1.5), "rate"), (dict(rate=nan), "rate"), (dict(fallback=0), "fallback"), (dict(key="0.18"), "key must be a number")):
        with pytest.raises(E, match=message):
            fm.make_meter(**kw)
    m = fm.make_meter(permille=900, rate=0.5)
    assert (m.key, m.permille, m.e_min, m.e_max, m.rate, m.fallback) == (f32(0.18), 900, 2.0 ** -10, 2.0 ** 10, 0.5, 1.0)
    for kw, message in ((dict(curve="aces"), "curve must be one of"), (dict(curve=5), "curve must be one of"), (dict(curve="reinhard", white=0), "white"),
                        (dict(curve="reinhard", white=nan), "white"), (dict(dither=1), "dither must be True or False"),
                        (dict(curve="reference", dither=True), "reference curve"), (dict(curve="reference", n_lut=16), "reference curve"),
                        (dict(exposure="1"), "exposure must be a number")):
        with pytest.raises(E, match=message):
            fm.make_params(**kw)
    p = fm.make_params(2.0, "filmic", dither=True)
    assert (p.exposure, p.curve, p.white, p.n_lut, p.dither) == (2.0, 3, inf, 0, 1)
    d = fm.make_params()
    assert (d.exposure, d.curve, d.n_lut, d.dither) == (1.0, 0, 0, 0)
    for bad in (None, np.zeros((4, 4, 3), f32), [[1.0, 2.0, 3.0]]):
        for fn in (fm.histogram, fm.develop):
            with pytest.raises(E, match="color must be a contiguous torch.float32 CUDA tensor"):
                fn(bad)
    with pytest.raises(E, match="hist must be an int32 CUDA tensor"):
        fm.expose(np.zeros(2048, np.int32))
    with pytest.raises(E, match="unknown meter parameter"):
        fm.expose(None, speed=2)
    # tables
    for bad in (1, 65537, 2.0, True):
        with pytest.raises(E, match="2..65536"):
            fm.srgb_lut(bad)
    with pytest.raises(E, match="g must be"):
        fm.gamma_lut(0)
    s = fm.srgb_lut()
    assert s.dtype == f32 and s.shape == (4096,) and s[0] == 0 and s[-1] == 1 and (np.diff(s) > 0).all()
    assert abs(float(fm.srgb_lut(256)[128]) - 0.7359) < 1e-3 and np.allclose(fm.gamma_lut(2.0, 5), np.sqrt(np.linspace(0, 1, 5)), atol=1e-7)
    assert np.array_equal(fm.gamma_lut(1.0, 2), np.array([0, 1], f32))
    # Film
    for kw, message in ((dict(curve="aces"), "curve must be one of"), (dict(lut=np.zeros(1, f32)), "2..65536"), (dict(lut=np.zeros((2, 2), f32), curve="atan"), "2..65536"),
                        (dict(lut=fm.srgb_lut(16)), "reference curve"), (dict(dither=True), "reference curve"), (dict(auto=True), "auto must be None or a dict"),
                        (dict(auto=dict(permille=0)), "permille"), (dict(auto=dict(gain=1)), "unknown meter parameter"), (dict(curve="reinhard", white=-1), "white")):
        with pytest.raises(E, match=message):
            sqt.Film(**kw)
    f = sqt.Film(curve="filmic", lut=fm.srgb_lut(64), dither=True, auto=dict(key=0.2))
    assert f.exposure_state is None
    f.exposure_state = 2.5
    assert f.exposure_state == 2.5
    f.reset()
    assert f.exposure_state is None
    assert sqt.Film is fm.Film and callable(sqt.Film())
    # the drivers refuse a film that is none before they look at the scene
    render = importlib.import_module("squigly-trace_amd.render")
    with pytest.raises(ValueError, match="film must be None or a Film"):
        next(render.render_adaptive(None, None, 8, (8, 8), 0.1, denoise=True, film="filmic"))
    with pytest.raises(ValueError, match="film needs denoise"):
        next(render.render_adaptive(None, None, 8, (8, 8), 0.1, film=sqt.Film()))
    with pytest.raises(ValueError, match="film must be None or a Film"):
        next(render.render_sequence(None, [sqt.Camera()], 4, (48, 64), film=1.0))
    with pytest.raises(ValueError, match="film must be None or a Film"):
        sqt.Temporal(None, 48, 64, 16, film="atan")


def test_cli_film_flags(sqt, tmp_path):
    cli = importlib.import_module("squigly-trace_amd.cli")
    seq = tmp_path / "move.cams"
    seq.write_text("0 7 0.75\n1.5707963267948966 0 -0.09817477042468103\n" * 2)
    S, A = ["--sequence", str(seq)], ["--adaptive", "0.5", "--denoise"]
    a = cli.parse_args(S + ["--film", "filmic", "--srgb", "--dither", "--auto-exposure"])
    assert (a.film, a.srgb, a.dither, a.auto_exposure, a.exposure, a.white) == ("filmic", True, True, 0.18, None, None)
    f = cli.film_of(a)
    assert isinstance(f, sqt.Film) and f.curve == "filmic" and f.dither is True and f.lut.shape == (4096,)
    assert f.auto == dict(key=0.18, rate=cli.AUTO_EXPOSURE_RATE)
    a = cli.parse_args(A + ["--film", "reinhard", "--white", "4", "--exposure", "2.5"])
    f = cli.film_of(a)
    assert (f.curve, f.white, f.exposure, f.auto, f.lut) == ("reinhard", 4.0, 2.5, None, None)
    assert cli.film_of(cli.parse_args(A + ["--film", "atan", "--auto-exposure", "0.3"])).auto == dict(key=0.3, rate=1.0)
    assert cli.film_of(cli.parse_args(A + ["--film", "reference"])).curve == "reference"
    assert cli.film_of(cli.parse_args(A)) is None and cli.film_of(cli.parse_args([])) is None and cli.parse_args([]).film is None
    for bad in (["--film", "filmic"], ["--film", "filmic", "--adaptive", "0.5"], ["--film", "filmic", "--cast"], ["--film", "filmic", "--views", str(seq)],
                ["--film", "filmic", "--aa"], ["--film", "filmic", "--preview-every", "2"], ["--film", "filmic", "--denoise"],
                S + ["--film", "aces"], S + ["--exposure", "2"], S + ["--auto-exposure"], S + ["--white", "2"], S + ["--srgb"], S + ["--dither"],
                S + ["--film", "reference", "--srgb"], S + ["--film", "reference", "--dither"], S + ["--film", "filmic", "--white", "2"],
                S + ["--film", "reinhard", "--white", "0"], S + ["--film", "atan", "--exposure", "0"], S + ["--film", "atan", "--exposure", "inf"],
                S + ["--film", "atan", "--exposure", "2", "--auto-exposure"], S + ["--film", "atan", "--auto-exposure", "-1"]):
        with pytest.raises(SystemExit):
            cli.parse_args(bad)


# ---- the restatement, and the one text for host and device against it ----
@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """tests/film_main.cpp built twice: plainly, and with -fsanitize=address,undefined (the runtimes inside the program)."""
    d = tmp_path_factory.mktemp("film_main")
    src = os.path.join(ROOT, "tests", "film_main.cpp")
    plain, san = str(d / "film_main"), str(d / "film_main_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", src, "-o", plain])
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", src, "-o", san], stderr=subprocess.DEVNULL)
    return plain, san


def words(a):
    return ["%08x" % int(u) for u in np.ascontiguousarray(a, f32).reshape(-1).view(np.uint32)]


def run_both(programs, args):
    outs = []
    for exe in programs:
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True)
        assert r.returncode == 0 and r.stderr == b"", (exe, r.returncode, r.stderr[-2000:])
        outs.append(r.stdout.decode().splitlines())
    assert outs[0] == outs[1]
    return outs[0]


LUTS = {"none": None, "two": np.array([0.25, 0.75], f32), "srgb": None, "odd": None}


def lut_named(fm, name):
    if name == "srgb":
        return fm.srgb_lut(4096)
    if name == "odd":                                         # not monotone, outside 0..1, an infinite entry at the far end
        t = np.cos(np.arange(7, dtype=f32)).astype(f32) * f32(1.5)
        t[-1] = np.inf
        return t
    return LUTS[name]


def test_edge_values_hold_every_edge():
    e = R.edge_values()
    assert np.isnan(e).any() and (e == inf).any() and (e == -inf).any() and (e < 0).any() and (e > 1).any()
    assert any(v == 0 and np.signbit(v) for v in e) and any(v == 0 and not np.signbit(v) for v in e)
    sub = e[(e > 0) & (e < f32(2.0) ** f32(-126))]
    assert len(sub) >= 3
    s = R.slot(e)
    assert s.min() == 0 and s.max() == 2047 and 2039 in s and {1, 7, 8, 9, 1015, 1016} <= set(s.tolist())
    # the boundaries 2^k: the value below falls in the slot before
    for k in (-20, -1, 0, 1, 7, 127):
        p = f32(2.0) ** f32(k)
        assert R.slot(p) == (k + 127) * 8 and R.slot(np.nextafter(p, f32(0))) == (k + 127) * 8 - 1 and R.slot(np.nextafter(p, f32(inf))) == (k + 127) * 8
    assert R.slot(f32(2.0) ** f32(-126)) == 8 and R.slot(np.nextafter(f32(2.0) ** f32(-126), f32(0))) == 7        # the largest subnormal
    assert list(R.slot(np.array([0.0, -0.0, nan, -1.0, -inf, 1e-45, inf, 3.4028235e38], f32))) == [0, 0, 0, 0, 0, 0, 2047, 2039]
    t = R.value_table(400, 1)
    assert t.shape == (400, 3) and (t.max(-1) == 0).any() and np.isnan(t).any()


CASES = [(curve, lut, dither) for curve in R.CURVES[1:] for lut in ("none", "two", "srgb", "odd") for dither in (False, True)] + [("reference", "none", False)]


@pytest.mark.parametrize("curve, lut, dither", CASES, ids=[f"{c}-{t}-{'dither' if d else 'plain'}" for c, t, d in CASES])
def test_the_pixel_text_is_the_restatement(fm, O, programs, curve, lut, dither):
    """Every edge value in every place of a pixel, under an exposure that is no power of two and a white inside the range: the bytes
    and the display values of csrc/sq_film_pixel.h, compiled by g++ with and without the sanitizers, against the numpy restatement."""
    table = lut_named(fm, lut)
    cols = 13                                                  # not a multiple of 8: the dither's rows and columns both wrap
    px = R.value_table(26 * cols, 5)
    for e, white in ((1.0, inf), (0.7, 2.5)):
        rgb, disp = R.develop(O, px.reshape(-1, cols, 3), e, curve, white, table, dither)
        args = ["develop", R.CURVES.index(curve), int(dither), cols] + words([e]) + words([white]) + [0 if table is None else len(table)]
        lines = run_both(programs, args + ([] if table is None else words(table)) + words(px))
        assert len(lines) == len(px)
        got = np.array([ln.split() for ln in lines])
        got_rgb = got[:, :3].astype(np.int64).astype(np.uint8)
        got_disp = np.array([[int(w, 16) for w in row] for row in got[:, 3:]], np.uint32).view(f32)
        assert np.array_equal(got_rgb, rgb.reshape(-1, 3)), np.argwhere(got_rgb != rgb.reshape(-1, 3))[:5]
        assert same(got_disp, disp.reshape(-1, 3))
        if curve != "reference":
            assert len(np.unique(rgb)) > 20


def test_restatement_edges(fm, O):
    """What the contract says in words, of the restatement itself."""
    c = np.array([[[0, 0, 0], [nan, 1, 1], [inf, 1, 1], [-1, -2, -3], [0.5, 0.25, 0.125], [3.0, 2.0, 1.0], [1e-45, 0, 0], [-0.0, 0.0, -0.0]]], f32)
    # curve 0 at exposure 1 is the renderer's tonemap: black (mx == 0, 0 / 0) and NaN come out 0, and a component over 1 wraps
    rgb, disp = R.develop(O, c)
    assert np.array_equal(rgb, np.array([[O.tonemap(tuple(float(v) for v in p)) for p in c[0]]], np.uint8))
    assert (rgb[0, 0] == 0).all() and np.isnan(disp[0, 0]).all() and (rgb[0, 1] == 0).all() and (rgb[0, 7] == 0).all()
    big = np.array([[[2000.0, 1.0, 1.0]]], f32)
    # atan(1000.5) / (pi / 2) * 255 = 254.84: the reference floors, the atan curve rounds
    assert R.develop(O, big)[0][0, 0, 0] == 254 and R.develop(O, big, 1.0, "atan")[0][0, 0, 0] == 255
    # values over 1 come from a negative component: mx = 0.001, lightness = -500, intensity / mx = -998.7, green = 998704.9, and
    # floor(998704.9 * 255) wraps mod 256 under curve 0 where the atan curve clamps; red and blue are -0.9987 and wrap to 256 - 255
    w = np.array([[[0.001, -1000.0, 0.001]]], f32)
    ref, d = R.develop(O, w)
    assert d[0, 0, 1] > 9e5 and ref[0, 0].tolist() == list(O.tonemap((0.001, -1000.0, 0.001)))
    assert ref[0, 0, 1] == int(np.floor(np.float64(f32(d[0, 0, 1] * f32(255))))) % 256 and ref[0, 0, 0] == 1
    assert R.develop(O, w, 1.0, "atan")[0][0, 0].tolist() == [0, 255, 0]
    # the clamping curves give 0 for NaN, negatives and -0, 255 for +inf
    for curve in ("atan", "reinhard", "filmic", "linear"):
        rgb, _ = R.develop(O, c, 1.0, curve)
        assert (rgb[0, 0] == 0).all() and rgb[0, 1, 0] == 0 and (rgb[0, 7] == 0).all(), curve
        # a negative pixel is an input like any other: it stays negative under the atan and linear curves, and comes out positive
        # where a curve divides by something negative (Reinhard: L = -2, Ld = 2, s = -1; the filmic fit: 2.48 / 1.98 at v = -1)
        assert (rgb[0, 3] == (0 if curve in ("atan", "linear") else 255)).all(), curve
    assert R.develop(O, np.array([[[inf, inf, inf]]], f32), 1.0, "linear")[0].tolist() == [[[255, 255, 255]]]
    assert R.develop(O, c, 1.0, "linear")[0][0, 4].tolist() == [128, 64, 32]          # 0.5 * 255 + 0.5 = 128.0, 64.25, 32.375
    # plain Reinhard is white = inf, and a finite white maps L == white to 1
    plain = R.develop(O, c, 1.0, "reinhard")[1]
    L = R.luminance(c)[0, 4]
    assert same(plain[0, 4], (L / (f32(1) + L)) / L * c[0, 4])
    g = np.array([[[4.0, 4.0, 4.0]]], f32)
    assert R.develop(O, g, 1.0, "reinhard", 4.0)[1].tolist() == [[[1.0, 1.0, 1.0]]]
    # a table's ends, n_lut = 2, and its clamp
    two = np.array([0.25, 0.75], f32)
    assert R.table(two, np.array([-1, 0, -0.0, nan, 0.5, 1, 2, inf], f32)).tolist() == [0.25, 0.25, 0.25, 0.25, 0.5, 0.75, 0.75, 0.75]
    s = fm.srgb_lut(4096)
    assert R.table(s, np.array([0, 1, 1.5], f32)).tolist() == [0.0, 1.0, 1.0] and abs(float(R.table(s, f32(0.5))) - 0.7354) < 1e-3
    # dither: thresholds 1/128 .. 127/128, each 64 times in 64 x 64, and a mid grey splits between two neighbouring bytes
    flat = np.full((64, 64, 3), 100.5 / 255, f32)
    d = R.develop(O, flat, 1.0, "linear", dither=True)[0]
    assert set(np.unique(d).tolist()) == {100, 101} and abs(int((d == 101).sum()) - d.size // 2) <= 3 * 64
    assert (R.develop(O, flat, 1.0, "linear")[0] == 101).all()


def test_the_expose_chain(fm, programs):
    """M == 0 with and without a previous exposure, the rank at permille 1 / 500 / 1000, both clamps, rate 0 and 1 and in between:
    the restatement in words, and csrc/sq_film_pixel.h's serial scan against it."""
    h = np.zeros(R.SLOTS, np.int64)
    mid = lambda s: np.array([(s << 20) | 0x80000], np.uint32).view(f32)[0]  # noqa: E731
    cases = []

    def both(hist, prev, **meter):
        want = R.expose(hist, prev, **meter)
        m = dict(R.METER, **meter)
        pairs = [v for s in np.nonzero(hist)[0] for v in (int(s), int(hist[s]))]
        args = ["expose"] + words([m["key"]]) + [m["permille"]] + words([m["e_min"]]) + words([m["e_max"]]) + words([m["rate"]]) + words([m["fallback"]])
        cases.append((args + [0 if prev is None else 1] + words([0.0 if prev is None else prev]) + pairs, want))
        return want

    # nothing metered: slots 0 and 2047 do not count
    h[0], h[2047] = 1000, 7
    assert both(h, None) == 1.0 and both(h, None, fallback=3.5) == 3.5 and both(h, 2.25) == 2.25
    for bad in (0.0, -1.0, nan, inf):
        assert both(h, bad, fallback=0.5) == 0.5
    # one slot: the exposure brings its middle to the key
    h[1016] = 10                                             # 1.0 .. 1.125, an eighth of a stop: Lp = 1.0625
    assert both(h, None) == f32(0.18) / mid(1016) and mid(1016) == f32(1.0625)
    # the rank: 100 pixels in slot 1000, 100 in 1016, 1 in 1040
    h[1000], h[1016], h[1040] = 100, 100, 1
    assert both(h, None, permille=1) == f32(0.18) / mid(1000)
    assert both(h, None, permille=497) == f32(0.18) / mid(1000)          # (201 * 497 + 999) / 1000 = 100
    assert both(h, None, permille=498) == f32(0.18) / mid(1016)          # ... 101
    assert both(h, None, permille=500) == f32(0.18) / mid(1016)
    assert both(h, None, permille=995) == f32(0.18) / mid(1016)          # (201 * 995 + 999) / 1000 = 200: the rank rounds up
    assert both(h, None, permille=996) == f32(0.18) / mid(1040) and both(h, None, permille=1000) == f32(0.18) / mid(1040)
    # the clamps
    assert both(h, None, e_max=0.125) == 0.125 and both(h, None, e_min=0.5) == 0.5 and both(h, None, e_min=0.25, e_max=0.25) == 0.25
    # the rate
    t = f32(0.18) / mid(1016)
    assert both(h, 2.0, rate=0.0) == 2.0 and both(h, 2.0, rate=1.0) == f32(f32(2.0) + f32(t - f32(2.0)))
    assert both(h, 2.0, rate=0.25) == f32(f32(2.0) + f32(f32(0.25) * f32(t - f32(2.0))))
    assert both(h, nan, rate=0.25) == t and both(h, 0.0, rate=0.0) == t and both(h, inf, rate=0.5) == t
    # the ends of the scan, and counts whose sum passes 2^32
    e = np.zeros(R.SLOTS, np.int64)
    e[1] = 1
    assert both(e, None, e_max=3e38) == f32(0.18) / mid(1) and both(e, None) == 1024.0      # a subnormal middle: 2.2e-39
    e[1], e[2046] = 0, 5
    assert np.isnan(both(e, None))                            # slot 2046 holds no float: its "middle" is a NaN, and so is the exposure
    e[2046], e[2039] = 0, 5
    assert both(e, None, e_min=1e-44) == f32(0.18) / mid(2039) and both(e, None, e_min=1e-38) == f32(1e-38)       # 5.5e-40, a subnormal
    big = np.zeros(R.SLOTS, np.int64)
    big[900], big[1100], big[1101] = 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1
    assert both(big, None, permille=667, e_min=1e-9) == f32(0.18) / mid(1101) and both(big, None, permille=666, e_min=1e-9) == f32(0.18) / mid(1100)
    assert both(big, None, permille=667) == f32(2.0 ** -10)
    for args, want in cases:
        (line,) = run_both(programs, args)
        got = np.array([int(line, 16)], np.uint32).view(f32)
        assert same(got, np.array([want], f32)), (args[:10], got, want)


def test_slots_of_the_pixel_text(programs):
    px = R.value_table(700, 9)
    lines = run_both(programs, ["slots"] + words(px))
    assert [int(v) for v in lines] == R.slot(R.luminance(px)).tolist()
    img = R.slot_image(37, 70, 3)
    hist = R.histogram(img)
    assert hist.sum() == 37 * 70 and (hist[:2040] > 0).all() and (hist[2040:2047] == 0).all() and hist[2047] >= 2 and hist[0] >= 4
