"""The denoiser without a GPU: the library's surface (exports, ids, refusals, workspace size), the variance formula on hand-worked
pixels, and the quality of the specified filter -- the numpy restatement -- on the project's own scene."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import denoise_restatement as R
import library_surface as LS
from denoise_room import room
from render_options import THREADS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NO_DEVICE = 1 << 20         # a device number no machine has: a call the checks let through by mistake fails there, before any launch


@pytest.fixture(scope="module")
def dn(sqt):
    mod = importlib.import_module("squigly-trace_amd.denoise")
    mod.lib()
    return mod


def test_header_functions_are_exported(dn):
    declared = LS.check_exports(dn, "squigly_denoise.h", "sq_denoise_")      # (and nothing of the other libraries' leaks out of this one)
    assert {"sq_denoise_device", "sq_denoise_variance_device", "sq_denoise_workspace_bytes", "sq_denoise_last_error"} <= declared


def test_main_library_did_not_gain_the_denoiser(sqt):
    for h in ("squigly_hip.h", "squigly_host.h"):
        assert "sq_denoise" not in open(os.path.join(ROOT, "include", h)).read(), h
    assert not [s for s in sqt.EXPORTED_SYMBOLS if "denoise" in s]
    nm = subprocess.check_output(["nm", "-D", "--defined-only", sqt.LIB_PATH]).decode()
    assert "denoise" not in nm and "sq_dn_" not in nm


def test_ids_are_separate(dn, sqt, tmp_path):
    b = LS.build_module()
    assert "sq_denoise.hip" not in LS.files(b, "main") and "../../include/squigly_denoise.h" not in LS.files(b, "main")
    assert dn.build_id() == b.lib_source_id(b.LIBS["denoise"]) != b.source_id()
    assert sqt.build_id() == b.source_id()
    # every id reads only its own lists: in a copy of csrc/ in which the filter's source differs, the filter's id moves and no other
    LS.check_ids(b, "denoise", dn, sqt, tmp_path, [("sq_denoise.hip", {"denoise"}), ("../../include/squigly_denoise.h", {"denoise"})])


def test_workspace_bytes_is_monotone(dn):
    wb = dn.workspace_bytes
    sizes = [1, 2, 3, 15, 16, 17, 63, 64, 65, 255, 1080, 1920, 4096, 46340]
    for r in sizes:
        for c0, c1 in zip(sizes, sizes[1:]):
            assert 0 < wb(r, c0) <= wb(r, c1) and wb(c0, r) <= wb(c1, r)
    assert wb(1920, 1080) == wb(1080, 1920) >= 1920 * 1080 * 16 * 4
    assert wb(0, 5) == wb(5, 0) == wb(-1, 5) == 0
    assert wb(2 ** 31 - 1, 1) > 0 and wb(46341, 46341) == 0 and wb(2 ** 31 - 1, 2) == 0


# ---- refusals: nothing here reaches a device, the pointers are numbers that are never followed ----
N_PIX = 6 * 5
BUF = {name: 0x10000000 + i * 0x100000 for i, name in enumerate(("color", "var", "tri", "normal", "point", "out", "out_var", "work"))}


def call(dn, rows=6, cols=5, params=None, work_bytes=None, null_params=False, **ptr):
    p = dict(sigma_p=0.05)
    p.update(params or {})
    P = dn.Params(p.get("passes", 5), p.get("sigma_l", 4.0), p.get("eps_l", 1e-3), p["sigma_p"], p.get("normal_squarings", 3), p.get("form", 0))
    a = {**BUF, **ptr}
    wb = dn.workspace_bytes(rows, cols) if work_bytes is None else work_bytes
    rc = dn.lib().sq_denoise_device(NO_DEVICE, rows, cols, a["color"], a["var"], a["tri"], a["normal"], a["point"],
                                    None if null_params else C.byref(P), a["out"], a["out_var"], a["work"], wb, None)
    return rc, dn.lib().sq_denoise_last_error().decode()


REFUSALS = [
    (dict(color=None), "null argument"), (dict(tri=None), "null argument"), (dict(normal=None), "null argument"),
    (dict(point=None), "null argument"), (dict(out=None), "null argument"), (dict(work=None), "null argument"),
    (dict(null_params=True), "null argument"),
    (dict(rows=0), "at least 1"), (dict(cols=0), "at least 1"), (dict(rows=-3), "at least 1"),
    (dict(rows=46341, cols=46341, work_bytes=1 << 40), "exceed 2\\^31 - 1"),
    (dict(params={"passes": 0}), "passes"), (dict(params={"passes": 9}), "passes"),
    (dict(params={"normal_squarings": -1}), "normal_squarings"), (dict(params={"normal_squarings": 9}), "normal_squarings"),
    (dict(params={"form": -1}), "form"), (dict(params={"form": 3}), "form"),
    (dict(params={"sigma_l": 0.0}), "sigma_l"), (dict(params={"sigma_l": float("nan")}), "sigma_l"), (dict(params={"sigma_l": -1.0}), "sigma_l"),
    (dict(params={"sigma_p": 0.0}), "sigma_p"), (dict(params={"sigma_p": float("nan")}), "sigma_p"),
    (dict(params={"eps_l": -1e-3}), "eps_l"), (dict(params={"eps_l": float("nan")}), "eps_l"),
    (dict(var=None), "d_out_var needs d_var"),
    (dict(work_bytes=6 * 5 * 64 - 1), "too small"), (dict(work_bytes=0), "too small"),
    (dict(work=BUF["work"] + 4), "16-byte aligned"),
    (dict(out=BUF["color"] + 12), "d_color and d_out overlap"),                 # shifted by a pixel: not the allowed d_out == d_color
    (dict(out_var=BUF["var"] + 4), "d_var and d_out_var overlap"),
    (dict(out=BUF["normal"]), "d_normal and d_out overlap"), (dict(out=BUF["point"]), "d_point and d_out overlap"),
    (dict(out=BUF["tri"]), "d_tri and d_out overlap"), (dict(out_var=BUF["color"]), "d_color and d_out_var overlap"),
    (dict(color=BUF["normal"]), "d_color and d_normal overlap"),
    (dict(work=BUF["out"] - 16), "d_out and d_work overlap"), (dict(color=BUF["work"] + 6 * 5 * 64 - 16), "d_color and d_work overlap"),
    (dict(out=BUF["out_var"] - 4), "d_out and d_out_var overlap"),
]


@pytest.mark.parametrize("kw, message", REFUSALS, ids=[f"{i:02d}-{m[:12]}" for i, (_, m) in enumerate(REFUSALS)])
def test_refusals_need_no_gpu(dn, kw, message):
    rc, err = call(dn, **kw)
    assert rc != 0 and re.search(message, err), err


def test_what_is_allowed_gets_past_the_checks(dn):
    """d_out == d_color, d_out_var == d_var and a call without variance pass every check: on a device that does not exist they
    fail at the first runtime call, and with its message."""
    for kw in (dict(), dict(out=BUF["color"], out_var=BUF["var"]), dict(var=None, out_var=None), dict(out_var=None)):
        rc, err = call(dn, **kw)
        assert rc != 0 and "hipSetDevice" in err, err


def test_variance_refusals(dn):
    L = dn.lib()
    s, q, c, v = 0x1000000, 0x2000000, 0x3000000, 0x4000000
    cases = [((10, None, q, c, v), "null"), ((10, s, None, c, v), "null"), ((10, s, q, None, v), "null"), ((10, s, q, c, None), "null"),
             ((-1, s, q, c, v), "negative"), ((10, s, q, c, s + 8), "d_var and d_sum overlap"), ((10, s, q, c, c), "d_var and d_count overlap")]
    for (n, *ptrs), message in cases:
        assert L.sq_denoise_variance_device(NO_DEVICE, n, *ptrs, None) != 0
        assert message in L.sq_denoise_last_error().decode()
    assert L.sq_denoise_variance_device(NO_DEVICE, 0, s, q, c, v, None) == 0         # no pixel: nothing to enqueue


def test_python_refusals(dn):
    with pytest.raises(dn.N.SquiglyError, match="sigma_p is required"):
        dn.make_params()
    with pytest.raises(dn.N.SquiglyError, match="unknown denoise parameter"):
        dn.make_params(sigma_p=0.1, sigma=3)
    with pytest.raises(dn.N.SquiglyError, match="form must be one of"):
        dn.make_params(sigma_p=0.1, form="fast")
    p = dn.make_params(sigma_p=0.1, form="tiled", passes=3)
    assert (p.passes, p.form, p.normal_squarings) == (3, 2, 3) and p.sigma_l == 4.0
    assert [dn.lib().sq_denoise_pass_form(i) in (1, 2) for i in range(8)] == [True] * 8
    assert dn.lib().sq_denoise_pass_form(8) == dn.lib().sq_denoise_pass_form(-1) == -1


def test_default_sigma_p_is_half_a_percent_of_the_diagonal(dn, product_scene):
    bih, _, _ = product_scene
    b = bih.bounds.astype(np.float64)
    assert abs(dn.default_sigma_p(bih.bounds) - 0.005 * np.linalg.norm(b[3:] - b[:3])) < 1e-9
    assert abs(dn.default_sigma_p(bih.bounds) - 0.0353) < 1e-4            # the room; the prototype's 0.05 is 0.7 % of it
    assert dn.default_sigma_p([0, 0, 0, 3, 4, 12]) == pytest.approx(0.065)


def test_cli_denoise_flag(sqt):
    cli = importlib.import_module("squigly-trace_amd.cli")
    assert cli.parse_args(["--adaptive", "0.5", "--denoise"]).denoise is True
    assert cli.parse_args(["--adaptive", "0.5", "--denoise", "2.5"]).denoise == 2.5
    assert cli.parse_args(["--adaptive", "0.5"]).denoise is None
    for bad in (["--denoise"], ["--adaptive", "0.5", "--denoise", "0"], ["--adaptive", "0.5", "--denoise", "nan"]):
        with pytest.raises(SystemExit):
            cli.parse_args(bad)
    render = importlib.import_module("squigly-trace_amd.render")
    assert render.denoise_options(True) == {} and render.denoise_options(2.5) == {"sigma_l": 2.5}
    assert render.denoise_options({"passes": 3}) == {"passes": 3}
    with pytest.raises(ValueError):
        render.denoise_options(-1.0)


# ---- the variance formula, by hand ----
def test_variance_on_hand_worked_pixels():
    nan = float("nan")
    #          count  sum                 sum of squares
    pixels = [(0, (5.0, 5.0, 5.0), (9.0, 9.0, 9.0)),          # no sample: +0
              (1, (2.0, 4.0, 8.0), (4.0, 16.0, 64.0)),        # one sample: l^2, l = 0.25*2 + 0.5*4 + 0.25*8 = 4.5
              (2, (2.0, 4.0, 0.0), (4.0, 10.0, 0.0)),         # means 1, 2, 0; d = 2-1, 5-4, 0 -> var 1, 1, 0 -> 0.0625 + 0.25
              (4, (4.0, 8.0, 4.0), (3.0, 20.0, 4.0)),         # means 1, 2, 1; d = -0.25 (-> +0), 1, 0 -> var 0, 1/3, 0
              (2, (nan, 2.0, 2.0), (1.0, 2.0, 2.0)),          # a NaN mean: d is NaN, compares false -> that channel's var is +0
              (-3, (1.0, 1.0, 1.0), (1.0, 1.0, 1.0))]         # a negative count is "< 1": +0
    c = np.array([p[0] for p in pixels], np.int32)
    s = np.array([p[1] for p in pixels], f32)
    q = np.array([p[2] for p in pixels], f32)
    v = R.variance(s, q, c)
    third = f32(1) / f32(3)
    want = np.array([0.0, 20.25, 0.3125, f32(0.25) * third, 0.0, 0.0], f32)
    assert v.dtype == f32 and np.array_equal(v.view(np.uint32), want.view(np.uint32)), (v, want)
    assert not np.signbit(v).any()
    # NaN in the sums of a one-sample pixel is the NaN the expression says
    assert np.isnan(R.variance(np.array([[nan, 1, 1]], f32), np.ones((1, 3), f32), np.array([1], np.int32)))[0]


# ---- the restatement itself ----
def test_restatement_edges():
    color, var, tri, nrm, pnt = R.synthetic(9, 11, seed=3)
    out, ov = R.denoise(color, tri, nrm, pnt, var, passes=3)
    bg = tri < 0
    assert bg.any() and (~bg).any()
    assert np.array_equal(out[bg].view(np.uint32), color[bg].view(np.uint32)) and np.array_equal(ov[bg].view(np.uint32), var[bg].view(np.uint32))
    assert not np.array_equal(out[~bg], color[~bg])
    # a lone valid pixel has one tap, itself, of weight K0 K0: the quotient gives the colour back up to rounding
    tri1 = np.full((3, 5), -1, np.int32)
    tri1[1, 2] = 7
    c, v, _, n, p = R.synthetic(3, 5, seed=4)
    c[1, 2], v[1, 2] = (1.0, 2.0, 3.0), 0.5
    o1, v1 = R.denoise(c, tri1, n, p, v, passes=2)
    assert np.allclose(o1[1, 2], (1.0, 2.0, 3.0), rtol=1e-6) and np.allclose(v1[1, 2], 0.5, rtol=1e-6)
    # all background: the identity, bit for bit; without var there is no variance
    o2, v2 = R.denoise(c, np.full((3, 5), -1, np.int32), n, p)
    assert v2 is None and np.array_equal(o2.view(np.uint32), c.view(np.uint32))


def test_quality_on_the_room(O, oracle_scene):
    """The specified filter, under the defaults, on the room at 48 x 64 and 16 spp against the oracle's 1024-spp frame over the hit
    pixels: mean squared error at most 0.5 x the noisy frame's, mean of err^2 / (ref^2 + 0.01) at most 0.2 x."""
    ob, cam, _ = oracle_scene
    rm = room(O, oracle_scene)
    avg16, _, _ = ob.render(cam, 16, 48, 64, threads=THREADS, want_rgb=False)
    assert np.array_equal(rm["avg"].view(np.uint32), avg16.view(np.uint32))          # the fold of the samples is render's avg
    var = R.variance(rm["sums"], rm["sums2"], rm["counts"])
    out, out_var = R.denoise(rm["avg"], rm["tri"], rm["normal"], rm["point"], var, **R.DEFAULTS)
    hit = rm["tri"] >= 0
    assert 0.3 < hit.mean() < 1.0              # the room is seen from outside: both kinds of pixel
    ref = rm["ref"].astype(np.float64)

    def errors(img):
        e2 = (img.astype(np.float64) - ref)[hit] ** 2
        return e2.mean(), (e2 / (ref[hit] ** 2 + 0.01)).mean()
    mse0, rel0 = errors(rm["avg"])
    mse1, rel1 = errors(out)
    print(f"noisy mse {mse0:.4f} rel {rel0:.4f}; filtered mse {mse1:.4f} rel {rel1:.4f}; ratios {mse1 / mse0:.3f} {rel1 / rel0:.3f}")
    assert mse1 <= 0.5 * mse0, (mse0, mse1)
    assert rel1 <= 0.2 * rel0, (rel0, rel1)
    assert np.isfinite(out_var[hit]).all() and (out_var[hit] >= 0).all()
