"""The glare stage without a GPU: the two calls' surface (exports, workspace bytes, refusals), the Python layer's and the command line's
refusals, the anchors of the contract on the numpy restatement, and the restatement held against tests/glare_main.cpp, a host program over
csrc/sq_glare_pixel.h (the text the kernels compile), built plainly and under the sanitizers."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import glare_restatement as R
import library_surface as LS
from bitcmp import same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NO_DEVICE = 1 << 20         # a device number no machine has: a call the checks let through by mistake fails there, before any launch
nan, inf = float("nan"), float("inf")


@pytest.fixture(scope="module")
def dn(sqt):
    mod = importlib.import_module("squigly-trace_amd.denoise")
    mod.lib()
    return mod


@pytest.fixture(scope="module")
def fm(sqt):
    return importlib.import_module("squigly-trace_amd.film")


def test_the_two_calls_are_declared_and_exported(dn):
    new = {"sq_denoise_glare_work_bytes", "sq_denoise_glare_device"}
    assert new <= LS.declared_in("squigly_denoise.h", "sq_denoise_") and new <= set(dn.EXPORTED_SYMBOLS) and new <= LS.exported_by(dn.LIB_PATH)
    assert not [n for n in LS.exported_by(dn.LIB_PATH) if "glare" in n and n not in new]
    b = LS.build_module()
    assert "sq_glare_pixel.h" in b.LIBS["denoise"]["headers"]
    assert not [n for n in b.LIBS if n != "denoise" and "sq_glare_pixel.h" in LS.files(b, n)]
    assert C.sizeof(dn.GlareParams) == 40


# ---- workspace bytes ----
def test_work_bytes_is_the_formula(dn):
    assert R.level_sizes(37, 70, 8) == [(19, 35), (10, 18), (5, 9), (3, 5), (2, 3), (1, 2), (1, 1), (1, 1)]
    assert R.work_bytes(1, 1, 8) == 16 * 8 and R.work_bytes(2, 2, 1) == 16 and R.work_bytes(3, 5, 2) == 16 * (2 * 3 + 1 * 2)
    table = [(1, 1, 8), (1, 1, 1), (1, 2, 3), (2, 1, 3), (3, 5, 2), (16, 16, 4), (17, 33, 5), (31, 32, 8), (33, 130, 3), (37, 70, 8), (300, 700, 5),
             (1080, 1920, 5), (4320, 7680, 8), (2 ** 31 - 1, 1, 8), (1, 2 ** 31 - 1, 1), (46340, 46340, 8)]
    for rows, cols, levels in table:
        assert dn.glare_work_bytes(rows, cols, levels) == R.work_bytes(rows, cols, levels) > 0, (rows, cols, levels)
        assert dn.glare_work_bytes(rows, cols, 0) == 0
    for rows, cols, levels in [(0, 5, 3), (5, 0, 3), (-1, 5, 3), (5, -7, 3), (46341, 46341, 3), (2 ** 31 - 1, 2, 1), (5, 5, -1), (5, 5, 9), (5, 5, 1 << 30)]:
        assert dn.glare_work_bytes(rows, cols, levels) == R.work_bytes(rows, cols, levels) == 0, (rows, cols, levels)
    # monotone in all three arguments
    for rows in range(1, 20):
        for cols in range(1, 20):
            for levels in range(0, 9):
                w = dn.glare_work_bytes(rows, cols, levels)
                assert w == R.work_bytes(rows, cols, levels)
                assert dn.glare_work_bytes(rows + 1, cols, levels) >= w and dn.glare_work_bytes(rows, cols + 1, levels) >= w
                assert levels == 8 or dn.glare_work_bytes(rows, cols, levels + 1) > w


# ---- refusals: nothing here reaches a device, the pointers are numbers that are never followed ----
BUF = {name: 0x10000000 + i * 0x100000 for i, name in enumerate(("color", "exposure", "out", "work"))}
ROWS, COLS = 6, 5
N = ROWS * COLS
PARAMS = dict(exposure=1.0, gain=(1.0, 1.0, 1.0), threshold=1.0, ceiling=16.0, levels=3, spread=0.5, strength=0.1, form=0)
NEED = R.work_bytes(ROWS, COLS, 3)


def call_glare(dn, rows=ROWS, cols=COLS, params=None, null_params=False, work_bytes=None, **ptr):
    a = {**BUF, **ptr}
    p = dict(PARAMS, **(params or {}))
    P = dn.GlareParams(p["exposure"], (C.c_float * 3)(*p["gain"]), p["threshold"], p["ceiling"], p["levels"], p["spread"], p["strength"], p["form"])
    wb = R.work_bytes(rows, cols, p["levels"]) if work_bytes is None else work_bytes
    rc = dn.lib().sq_denoise_glare_device(NO_DEVICE, rows, cols, a["color"], a["exposure"], None if null_params else C.byref(P), a["out"], a["work"],
                                          wb, None)
    return rc, dn.lib().sq_denoise_last_error().decode()


REFUSALS = [
    (dict(color=None), "null argument"), (dict(out=None), "null argument"), (dict(null_params=True), "null argument"),
    (dict(rows=0), "at least 1"), (dict(cols=0), "at least 1"), (dict(rows=-3), "at least 1"), (dict(rows=46341, cols=46341), "exceed 2\\^31 - 1"),
    (dict(params={"levels": -1}), "levels"), (dict(params={"levels": 9}), "levels"),
    (dict(params={"form": -1}), "form"), (dict(params={"form": 3}), "form"),
    (dict(params={"threshold": nan}), "threshold"), (dict(params={"threshold": -0.5}), "threshold"), (dict(params={"threshold": inf}), "threshold"),
    (dict(params={"ceiling": nan}), "ceiling"), (dict(params={"ceiling": inf}), "ceiling"), (dict(params={"ceiling": 1.0}), "ceiling"),
    (dict(params={"ceiling": 0.5}), "ceiling"), (dict(params={"threshold": 0.0, "ceiling": 0.0}), "ceiling"),
    (dict(params={"spread": nan}), "spread"), (dict(params={"spread": -1.0}), "spread"), (dict(params={"spread": inf}), "spread"),
    (dict(params={"strength": nan}), "strength"), (dict(params={"strength": -1.0}), "strength"), (dict(params={"strength": inf}), "strength"),
    (dict(work_bytes=NEED - 1), "too small"), (dict(work_bytes=0), "too small"), (dict(work=None), "d_work is required"),
    (dict(work=BUF["work"] + 8), "16-byte aligned"), (dict(work=BUF["work"] + 4), "16-byte aligned"),
    (dict(out=BUF["color"] + 4), "d_color and d_out overlap"), (dict(out=BUF["color"] + 12 * N - 4), "d_color and d_out overlap"),
    (dict(color=BUF["out"] + 12), "d_color and d_out overlap"),
    (dict(exposure=BUF["color"] + 8), "d_color and d_exposure overlap"), (dict(exposure=BUF["out"]), "d_exposure and d_out overlap"),
    (dict(exposure=BUF["work"] + NEED - 4), "d_exposure and d_work overlap"),
    (dict(work=BUF["color"] + 16), "d_color and d_work overlap"), (dict(color=BUF["work"] + NEED - 4), "d_color and d_work overlap"),
    (dict(work=BUF["out"] - 16), "d_out and d_work overlap"), (dict(out=BUF["work"] + NEED - 4), "d_out and d_work overlap"),
    (dict(out=BUF["color"], work=BUF["color"] + 16), "d_color and d_work overlap"),
    (dict(params={"levels": 0}, work=BUF["color"], work_bytes=64), "d_color and d_work overlap"),       # a workspace that is given is checked
]
ids_of = lambda cases: [f"{i:02d}-{m[:12]}" for i, (_, m) in enumerate(cases)]  # noqa: E731


@pytest.mark.parametrize("kw, message", REFUSALS, ids=ids_of(REFUSALS))
def test_glare_refusals_need_no_gpu(dn, kw, message):
    rc, err = call_glare(dn, **kw)
    assert rc != 0 and re.search(message, err) and "hipSetDevice" not in err, err


def test_what_is_allowed_gets_past_the_checks(dn):
    """d_out == d_color, no device exposure, levels = 0 without a workspace, buffers that start anywhere, a workspace larger than
    needed, the extreme parameters and values that are merely odd pass every check: on a device that does not exist they fail at the
    first runtime call, with its message."""
    cases = [call_glare(dn), call_glare(dn, out=BUF["color"]), call_glare(dn, exposure=None), call_glare(dn, color=BUF["color"] + 4, out=BUF["out"] + 8),
             call_glare(dn, params={"levels": 0}, work=None, work_bytes=0), call_glare(dn, params={"levels": 0}, work=BUF["work"] + 3, work_bytes=1),
             call_glare(dn, params={"levels": 8}), call_glare(dn, work_bytes=NEED + 1000), call_glare(dn, rows=1, cols=1, params={"levels": 8}),
             call_glare(dn, rows=2 ** 31 - 1, cols=1, params={"levels": 1}, color=0x1000000000, out=0x8000000000, work=0x10000000000),
             call_glare(dn, params={"form": 1}), call_glare(dn, params={"form": 2}),
             call_glare(dn, params={"exposure": nan, "gain": (nan, -1.0, inf)}), call_glare(dn, params={"threshold": 0.0, "ceiling": 1e-45}),
             call_glare(dn, params={"threshold": 3e38, "ceiling": 3.4e38, "spread": 0.0, "strength": 0.0}),
             call_glare(dn, params={"spread": 3e38, "strength": 3e38})]
    for i, (rc, err) in enumerate(cases):
        assert rc != 0 and "hipSetDevice" in err, (i, err)


def test_python_refusals(dn, fm, sqt):
    E = dn.N.SquiglyError
    bad = [(dict(gain=(1, 1)), "gain must be three numbers"), (dict(gain=2.0), "gain must be three numbers"), (dict(gain=(1, "1", 1)), "gain must be a number"),
           (dict(threshold=-1), "threshold"), (dict(threshold=nan), "threshold"), (dict(threshold=inf), "threshold"), (dict(threshold="1"), "threshold must be a number"),
           (dict(ceiling=1.0), "ceiling"), (dict(ceiling=inf), "ceiling"), (dict(ceiling=nan), "ceiling"), (dict(ceiling=1.0 + 1e-9), "ceiling"),
           (dict(ceiling=1e39), "ceiling"), (dict(levels=-1), "levels"), (dict(levels=9), "levels"), (dict(levels=2.0), "levels"), (dict(levels=True), "levels"),
           (dict(spread=-0.1), "spread"), (dict(spread=inf), "spread"), (dict(spread=nan), "spread"), (dict(strength=-0.1), "strength"),
           (dict(strength=1e39), "strength"), (dict(strength=nan), "strength")]
    for kw, message in bad:
        with pytest.raises(E, match=message):
            dn.make_glare_params(**kw)
    for kw, message in bad:
        if "gain" not in kw:
            with pytest.raises(E, match=message):
                sqt.Glare(**kw)
    for kw, message in ((dict(form="fast"), "form must be one of"), (dict(form=3), "form must be one of"), (dict(form=1.0), "form must be one of"),
                        (dict(exposure="1"), "exposure must be a number")):
        with pytest.raises(E, match=message):
            dn.make_glare_params(**kw)
    p = dn.make_glare_params(2.0, (1.5, 1.0, 0.5), form="tiled")
    assert (p.exposure, tuple(p.gain), p.threshold, p.ceiling, p.levels, p.spread, p.strength, p.form) == (2.0, (1.5, 1.0, 0.5), 1.0, 16.0, 5, 0.5, f32(0.1), 2)
    assert dn.GLARE_DEFAULTS == R.DEFAULTS and dn.MAX_GLARE_LEVELS == R.MAX_LEVELS
    for notcolor in (None, np.zeros((4, 4, 3), f32), [[1.0, 2.0, 3.0]]):
        with pytest.raises(E, match="color must be a contiguous torch.float32 CUDA tensor"):
            dn.glare(notcolor)
    # Glare: a value object
    g = sqt.Glare()
    assert g.params() == R.DEFAULTS and g == sqt.Glare(**R.DEFAULTS) and g != sqt.Glare(strength=0) and hash(g) == hash(sqt.Glare())
    assert sqt.Glare is fm.Glare and "strength=0.1" in repr(g)
    with pytest.raises(AttributeError):
        g.strength = 2.0
    assert sqt.Glare(0.0, 1e-3, 0, 0.0, 0.0).levels == 0 and sqt.Glare(levels=8, spread=3e38).spread == 3e38
    # Film(glare=, balance=)
    for kw, message in ((dict(glare=0.1), "glare must be None or a Glare"), (dict(glare=R.DEFAULTS), "glare must be None or a Glare"),
                        (dict(balance=1.0), "balance must be None or three numbers"), (dict(balance=(1, 2)), "balance must be None or three numbers"),
                        (dict(balance=(1, 2, "3")), "balance must be a number"), (dict(balance=(1, 2, 3, 4)), "balance must be None or three numbers")):
        with pytest.raises(E, match=message):
            sqt.Film(curve="filmic", **kw)
    f = sqt.Film(curve="filmic", glare=g, balance=(2, 1, 0.5))
    assert f.glare is g and f.balance == (2.0, 1.0, 0.5)
    plain = sqt.Film(curve="filmic")
    assert plain.glare is None and plain.balance is None


def test_cli_bloom_flags(sqt, tmp_path):
    cli = importlib.import_module("squigly-trace_amd.cli")
    seq = tmp_path / "move.cams"
    seq.write_text("0 7 0.75\n1.5707963267948966 0 -0.09817477042468103\n" * 2)
    S, A = ["--sequence", str(seq)], ["--adaptive", "0.5", "--denoise"]
    a = cli.parse_args(S + ["--film", "filmic", "--bloom"])
    assert (a.bloom, a.bloom_threshold, a.bloom_levels, a.white_balance) == (0.1, None, None, None)
    f = cli.film_of(a)
    assert f.glare == sqt.Glare() and f.balance is None
    f = cli.film_of(cli.parse_args(A + ["--film", "reinhard", "--bloom", "0.25", "--bloom-threshold", "2", "--bloom-levels", "3", "--white-balance", "1.5,1,0.75"]))
    assert f.glare == sqt.Glare(threshold=2.0, ceiling=32.0, levels=3, strength=0.25) and f.balance == (1.5, 1.0, 0.75)
    f = cli.film_of(cli.parse_args(S + ["--film", "atan", "--white-balance", "(-1,2,3)"]))
    assert f.glare is None and f.balance == (-1.0, 2.0, 3.0)
    assert cli.film_of(cli.parse_args(S + ["--film", "linear", "--bloom", "0", "--bloom-threshold", "0"])).glare == sqt.Glare(threshold=0.0, strength=0.0)
    plain = cli.film_of(cli.parse_args(S + ["--film", "filmic"]))
    assert plain.glare is None and plain.balance is None
    for bad in (S + ["--bloom"], S + ["--white-balance", "1,1,1"], S + ["--bloom-threshold", "2"], S + ["--bloom-levels", "3"],
                ["--film", "filmic", "--bloom"], A[:2] + ["--film", "filmic", "--bloom"],
                S + ["--film", "reference", "--bloom"], S + ["--film", "reference", "--white-balance", "1,1,1"],
                S + ["--film", "filmic", "--bloom-threshold", "2"], S + ["--film", "filmic", "--bloom-levels", "3"],
                S + ["--film", "filmic", "--bloom", "-1"], S + ["--film", "filmic", "--bloom", "inf"], S + ["--film", "filmic", "--bloom", "nan"],
                S + ["--film", "filmic", "--bloom", "--bloom-levels", "0"], S + ["--film", "filmic", "--bloom", "--bloom-levels", "9"],
                S + ["--film", "filmic", "--bloom", "--bloom-threshold", "-1"], S + ["--film", "filmic", "--bloom", "--bloom-threshold", "1e38"],
                S + ["--film", "filmic", "--white-balance", "1,1"], S + ["--film", "filmic", "--white-balance", "a,b,c"]):
        with pytest.raises(SystemExit):
            cli.parse_args(bad)


# ---- the anchors, on the restatement itself ----
def test_constant_frame_anchor():
    """A frame of constant 2.0 under e = 1, gain = 1, threshold = 1, ceiling = 4, levels = 3, spread = 0.5, strength = 0.25 is exactly
    2.4375 everywhere: b = 1, every level is 1 (the taps' weights sum to 1 exactly), A_1 = 1.5, A_0 = 1.75, 2 + 0.25 * 1.75."""
    for rows, cols in ((1, 1), (1, 2), (3, 5), (17, 33), (37, 70)):
        out = R.glare(np.full((rows, cols, 3), 2.0, f32), 1.0, (1, 1, 1), 1.0, 4.0, 3, 0.5, 0.25)
        assert out.shape == (rows, cols, 3) and out.dtype == f32 and (out == f32(2.4375)).all(), (rows, cols)


def test_interior_impulse_anchor():
    """A single pixel of 8.0 at (31, 30) of a black 64 x 64 frame: L = 8, m = 4, s = 3 / 8, b = 3.0; the down step spreads it over B_0
    with weights that sum to 1 / 4 -- one output in four sees a fine pixel with all its weight -- so 4 * sum(B_0) = 3.0 exactly."""
    px = np.zeros((64, 64, 3), f32)
    px[31, 30] = 8.0
    x = R.exposed(px, 1.0, (1, 1, 1))
    b = R.bright(x, 1.0, 4.0)
    assert (b[31, 30] == 3.0).all() and b.sum() == 9.0
    B0 = R.pyramid(x, 1.0, 4.0, 1)[0]
    assert B0.shape == (32, 32, 3)
    for ch in range(3):
        assert f32(4) * B0[..., ch].sum(dtype=np.float64) == 3.0
        assert np.count_nonzero(B0[..., ch]) == 4                     # a fine pixel is seen by two outputs each way


def test_restatement_edges():
    """What the contract says in words: every b lies in [0, ceiling] whatever the pixel holds; a poisoned pixel stays in its own pixel;
    all eight levels of a 37 x 70 frame are finite, and the frame reaches 1 x 1 at level 6."""
    px = R.random_frame(37, 70, 11)
    assert np.isnan(px).any() and np.isinf(px).any() and (px < 0).any() and (px == f32(1e30)).any()
    x = R.exposed(px, 0.7, (1.5, 1.0, 0.6))
    b = R.bright(x, 1.0, 16.0)
    assert np.isfinite(b).all() and (b >= 0).all() and (b <= 16).all() and (b == 16).any() and (b == 0).any() and ((b > 0) & (b < 16)).any()
    Bs = R.pyramid(x, 1.0, 16.0, 8)
    assert [p.shape[:2] for p in Bs] == R.level_sizes(37, 70, 8) and Bs[6].shape[:2] == (1, 1) == Bs[7].shape[:2]
    assert all(np.isfinite(p).all() and (p >= 0).all() and (p <= 16).all() for p in Bs)
    out = R.glare(px, 0.7, (1.5, 1.0, 0.6), levels=8)
    assert np.array_equal(np.isnan(out), np.isnan(x)) and np.array_equal(np.isinf(out), np.isinf(x))
    # levels = 0 is the exposed pixel, and strength 0 adds +0: only the sign of a zero can differ
    zero = R.glare(px, 0.7, (1.5, 1.0, 0.6), levels=5, strength=0.0)
    assert same(R.glare(px, 0.7, (1.5, 1.0, 0.6), levels=0), x) and np.array_equal(zero[~np.isnan(x)], x[~np.isnan(x)])
    # the bright pass in words
    t = R.bright(np.array([[1.0, 1.0, 1.0], [4.0, 4.0, 4.0], [32.0, 32.0, 32.0], [inf, 1, 1], [nan, 5, 5], [-8, 40, -8], [1e30, 1e30, 1e30]], f32), 1.0, 16.0)
    assert t[0].tolist() == [0, 0, 0] and t[1].tolist() == [3, 3, 3] and t[2].tolist() == [15, 15, 15] and t[3].tolist() == [0, 0, 0]
    assert t[4].tolist() == [0, 0, 0] and t[5].tolist() == [0, 16, 0] and np.abs(t[6] - 15).max() < 1e-4


# ---- the one text for host and device against the restatement ----
@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """tests/glare_main.cpp built twice: plainly, and with -fsanitize=address,undefined (the runtimes inside the program)."""
    d = tmp_path_factory.mktemp("glare_main")
    src = os.path.join(ROOT, "tests", "glare_main.cpp")
    plain, san = str(d / "glare_main"), str(d / "glare_main_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", src, "-o", plain])
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", src, "-o", san], stderr=subprocess.DEVNULL)
    return plain, san


def words(a):
    return ["%08x" % int(u) for u in np.ascontiguousarray(a, f32).reshape(-1).view(np.uint32)]


def unwords(rows):
    return np.array([[int(w, 16) for w in row] for row in rows], np.uint32).view(f32)


def run_both(programs, args):
    outs = []
    for exe in programs:
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True)
        assert r.returncode == 0 and r.stderr == b"", (exe, r.returncode, r.stderr[-2000:])
        outs.append(r.stdout.decode().splitlines())
    assert outs[0] == outs[1]
    return outs[0]


@pytest.mark.parametrize("e, gain, threshold, ceiling", [(1.0, (1.0, 1.0, 1.0), 1.0, 16.0), (0.7, (1.5, 1.0, 0.6), 0.25, 3.0), (2.0, (-1.0, 1.0, 1.0), 0.0, 1e-3)],
                         ids=["defaults", "balanced", "odd"])
def test_the_bright_pass_is_the_restatement(programs, e, gain, threshold, ceiling):
    """Every edge value -- NaN, +-inf, -0, negatives, subnormals, 1e30, values at and around the threshold and the ceiling -- in every
    channel position: the exposed pixel and its bright pass from csrc/sq_glare_pixel.h against the numpy restatement."""
    px = R.bright_table(threshold, ceiling)
    ev = R.bright_edge_values(threshold, ceiling)
    assert np.isnan(ev).any() and (ev == inf).any() and (ev == -inf).any() and any(v == 0 and np.signbit(v) for v in ev) and (ev == f32(1e30)).any()
    assert ((ev > 0) & (ev < f32(2.0) ** f32(-126))).any() and {f32(threshold), f32(ceiling)} <= set(ev.tolist())
    lines = run_both(programs, ["bright"] + words([e]) + words(gain) + words([threshold, ceiling]) + words(px))
    got = unwords([ln.split() for ln in lines])
    x = R.exposed(px, e, gain)
    b = R.bright(x, threshold, ceiling)
    assert got.shape == (len(px), 6) and same(got[:, :3], x) and same(got[:, 3:], b)
    assert np.isfinite(b).all() and (b >= 0).all() and (b <= f32(ceiling)).all() and len(np.unique(b)) > 8


def test_the_taps_are_the_restatement(programs):
    """The down step's four clamped taps for every output, and the up step's two clamped taps and weights for every fine coordinate,
    of the extents 1 .. 9."""
    lines = run_both(programs, ["taps", 9])
    want = []
    for n in range(1, 10):
        t = R.down_taps(n)
        want += [f"d {n} {o} {t[0][o]} {t[1][o]} {t[2][o]} {t[3][o]}" for o in range((n + 1) // 2)]
        i0, i1, a, b = R.up_taps(n, (n + 1) // 2)
        want += [f"u {n} {v} {i0[v]} {i1[v]} {words([a[v]])[0]} {words([b[v]])[0]}" for v in range(n)]
    assert lines == want
    assert "d 1 0 0 0 0 0" in lines and "u 1 0 0 0 3e800000 3f400000" in lines and "d 9 4 7 8 8 8" in lines and "u 9 8 3 4 3e800000 3f400000" in lines
    assert "u 9 1 0 1 3f400000 3e800000" in lines


FRAMES = [(1, 1, 8), (1, 2, 3), (2, 1, 3), (3, 5, 2), (7, 9, 0), (9, 7, 1), (17, 33, 3), (37, 70, 8)]


@pytest.mark.parametrize("rows, cols, levels", FRAMES, ids=[f"{r}x{c}-{n}" for r, c, n in FRAMES])
def test_the_whole_call_on_the_host_is_the_restatement(programs, rows, cols, levels):
    """The header's text composed level by level as the library enqueues it -- the up steps in place -- over a frame with NaN, inf,
    negative and 1e30 pixels: every bit of out against the restatement."""
    px = R.random_frame(rows, cols, 100 + rows) if rows * cols >= 40 else R.value_frame(rows, cols, 100 + rows)
    e, gain, t, c, spread, strength = 0.7, (1.5, 1.0, 0.6), 0.5, 8.0, 0.6, 0.3
    lines = run_both(programs, ["frame", rows, cols, levels] + words([e]) + words(gain) + words([t, c, spread, strength]) + words(px))
    got = unwords([ln.split() for ln in lines]).reshape(rows, cols, 3)
    assert same(got, R.glare(px, e, gain, t, c, levels, spread, strength))
