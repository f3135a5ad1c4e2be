"""CPU tests of the adaptive-sampling surface: the two entry points of the C-ABI, the refusals that come before any device work,
the argument checks of Adaptive and the CLI flags, and the numpy restatement of the stopping rule on hand-made pixels (the
renders themselves: tests/test_gpu_adaptive.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT


def _declarations():
    text = open(os.path.join(ROOT, "include", "squigly_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _params(name):
    decl = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", _declarations())
    assert decl, f"{name} is not declared in include/squigly_hip.h"
    return [p.split()[-1].lstrip("*") for p in decl.group(1).split(",")]


def test_header_declares_the_entry_points_and_the_library_exports_them(sqt):
    assert _params("sq_render_rows_device_masked") == ["s", "cam", "samples", "w", "h", "cast", "sh", "k_begin", "k_end", "d_mask",
                                                        "d_sum", "d_sum2", "d_count", "d_avg", "d_rgb", "hip_stream"]
    assert _params("sq_adaptive_update_device") == ["s", "n_pixels", "d_sum", "d_sum2", "d_count", "tol", "eps", "d_mask", "d_live",
                                                     "hip_stream"]
    nm = subprocess.check_output(["nm", "-D", "--defined-only", sqt.LIB_PATH]).decode()
    L = sqt.lib()
    for name, nargs in (("sq_render_rows_device_masked", 16), ("sq_adaptive_update_device", 10)):
        assert name in sqt.EXPORTED_SYMBOLS
        assert re.search(r" T " + name + "$", nm, flags=re.M)
        assert len(getattr(L, name).argtypes) == nargs
    assert L.sq_abi_version() == 1                                   # additions: the ABI stays compatible
    text = open(os.path.join(ROOT, "include", "squigly_hip.h")).read()
    assert "HEURISTIC" in text                                       # the header says what the rule is


def test_refusals_that_need_no_device(sqt):
    L = sqt.lib()
    cam = sqt.Camera()
    sh = sqt.Shard(8, 0, 1)
    one = C.c_void_p(16)                                             # never dereferenced: every call below is refused first
    for kb, ke, n in ((-1, 2, 4), (2, 2, 4), (3, 1, 4), (0, 5, 4)):
        assert L.sq_render_rows_device_masked(None, C.byref(cam), n, 8, 8, 0, sh, kb, ke, None, one, None, None, None, None, None) != 0
        assert b"bad sample range" in L.sq_last_error()
    assert L.sq_render_rows_device_masked(None, C.byref(cam), 4, 8, 8, 0, sh, 0, 4, None, None, None, None, one, None, None) != 0
    assert b"d_sum is required" in L.sq_last_error()
    assert L.sq_render_rows_device_masked(None, C.byref(cam), 4, 8, 8, 0, sh, 0, 4, None, one, None, None, one, None, None) != 0
    assert b"d_sum and d_avg" in L.sq_last_error()
    assert L.sq_render_rows_device_masked(None, C.byref(cam), 4, 8, 8, 0, sh, 0, 4, None, one, None, None, None, None, None) != 0
    assert b"null argument" in L.sq_last_error()
    for tol, eps in ((-1.0, 1.0), (0.5, -1.0), (float("nan"), 1.0), (0.5, float("nan"))):
        assert L.sq_adaptive_update_device(None, 4, None, None, None, tol, eps, None, None, None) != 0
        assert b"tol and eps" in L.sq_last_error()
    assert L.sq_adaptive_update_device(None, -1, None, None, None, 0.5, 1.0, None, None, None) != 0
    assert b"n_pixels" in L.sq_last_error()
    assert L.sq_adaptive_update_device(None, 4, None, None, None, 0.5, 1.0, None, None, None) != 0
    assert b"null argument" in L.sq_last_error()


def test_adaptive_checks_its_arguments_before_touching_a_device(sqt):
    ok = dict(samples=8, w=8, h=8, tol=0.5)
    bad = [dict(samples=0), dict(tol=-0.1), dict(tol=float("nan")), dict(eps=-1.0), dict(eps=float("nan")), dict(first=0),
           dict(step=0), dict(done=-1), dict(done=9), dict(done=4), dict(rule=3)]      # done=4 alone: resuming needs the tensors
    for kw in bad:
        a = {**ok, **kw}
        with pytest.raises(ValueError):
            sqt.Adaptive(None, None, a.pop("samples"), a.pop("w"), a.pop("h"), a.pop("tol"), **a)
    with pytest.raises(sqt.SquiglyError):
        sqt.Adaptive(None, None, 8, 8, 8, 0.5, shard=(2, 3, 3))


def test_cli_accepts_the_adaptive_flags_and_defaults_to_none():
    from importlib import import_module
    cli = import_module("squigly-trace_amd.cli")
    a = cli.parse_args([])
    assert a.adaptive is None and a.counts is None
    a = cli.parse_args(["--adaptive", "0.5", "--adaptive-first", "4", "--adaptive-step", "2", "--adaptive-eps", "0.25", "--counts", "c.npy"])
    assert (a.adaptive, a.adaptive_first, a.adaptive_step, a.adaptive_eps, a.counts) == (0.5, 4, 2, 0.25, "c.npy")
    a = cli.parse_args(["--adaptive", "0"])
    assert (a.adaptive, a.adaptive_first, a.adaptive_step, a.adaptive_eps) == (0.0, 8, 8, 1.0)
    for bad in (["--adaptive", "-1"], ["--adaptive", "nan"], ["--adaptive", "x"], ["--adaptive", "0.5", "--adaptive-first", "0"],
                ["--adaptive", "0.5", "--adaptive-step", "0"], ["--adaptive", "0.5", "--adaptive-eps", "-1"],
                ["--counts", "c.npy"], ["--adaptive", "0.5", "--preview-every", "2"]):
        with pytest.raises(SystemExit):
            cli.parse_args(bad)


def test_render_adaptive_is_exported_and_checks_before_a_scene_is_uploaded(sqt):
    for kw in (dict(tol=0.5, first=0), dict(tol=0.5, step=0), dict(tol=-1.0), dict(tol=0.5, eps=float("nan"))):
        gen = sqt.render_adaptive(None, None, 4, (8, 8), **kw)
        with pytest.raises(ValueError):
            next(gen)                                                 # refused before a scene is uploaded


def _rule(sqt, s, q, c, tol, eps, mask=None):
    s, q = np.asarray(s, np.float32).reshape(-1, 3), np.asarray(q, np.float32).reshape(-1, 3)
    c = np.asarray(c, np.int32).reshape(-1)
    mask = np.ones(len(c), np.uint8) if mask is None else np.asarray(mask, np.uint8)
    return sqt.rule_reference(s, q, c, mask, tol, eps)


def test_rule_restatement_on_hand_made_pixels(sqt):
    """1 = still live.  Every case is worked out by hand from the rule's text in include/squigly_hip.h."""
    inf, nan = float("inf"), float("nan")
    # constant samples r = 2 per channel, n = 4: s = 8, q = 16, lhs = 4 * 16 - 64 = 0 <= anything non-negative: converged
    assert _rule(sqt, [8, 8, 8], [16, 16, 16], [4], 0.5, 1.0).tolist() == [0]
    # all-zero pixel (it has seen only black): 0 <= 3 * 0.25 * (0 + 1 * 16): converged, at tol = 0 as well (0 <= 0)
    assert _rule(sqt, [0, 0, 0], [0, 0, 0], [4], 0.5, 1.0).tolist() == [0]
    assert _rule(sqt, [0, 0, 0], [0, 0, 0], [4], 0.0, 0.0).tolist() == [0]
    # n = 1: both sides are 0 for every finite sample, but one sample never converges; n = 0 neither
    assert _rule(sqt, [3, 3, 3], [9, 9, 9], [1], 0.5, 1.0).tolist() == [1]
    assert _rule(sqt, [0, 0, 0], [0, 0, 0], [0], 0.5, 1.0).tolist() == [1]
    # one bright sample of 100 among 8, red only: s = 100, q = 10000: lhs = 8 * 10000 - 10000 = 70000;
    # rhs sum = 10000 + 3 * 64 = 10192; 7 * 0.25 * 10192 = 17836 < 70000: live.  With tol = 2: 7 * 4 * 10192 >= 70000: converged
    assert _rule(sqt, [100, 0, 0], [10000, 0, 0], [8], 0.5, 1.0).tolist() == [1]
    assert _rule(sqt, [100, 0, 0], [10000, 0, 0], [8], 2.0, 1.0).tolist() == [0]
    # exact boundary, '<=': n = 2, samples 0 and 2 in one channel: s = 2, q = 4, L = 2 * 4 - 4 = 4; eps = 0: R = 4; tol = 1: 1 * 1 * 4 = 4
    assert _rule(sqt, [2, 0, 0], [4, 0, 0], [2], 1.0, 0.0).tolist() == [0]
    assert _rule(sqt, [2, 0, 0], [4, 0, 0], [2], 0.999, 0.0).tolist() == [1]
    # NaN anywhere compares false: live.  inf - inf = NaN as well
    assert _rule(sqt, [nan, 0, 0], [0, 0, 0], [4], 0.5, 1.0).tolist() == [1]
    assert _rule(sqt, [1, 1, 1], [1, nan, 1], [4], 0.5, 1.0).tolist() == [1]
    assert _rule(sqt, [inf, 0, 0], [inf, 0, 0], [4], 0.5, 1.0).tolist() == [1]
    # s * s overflows but q is finite: lhs = -inf <= +inf: converged (the comparison is taken as it falls)
    assert _rule(sqt, [3e38, 0, 0], [1e30, 0, 0], [4], 0.5, 1.0).tolist() == [0]
    # negative sums square like positive ones
    assert _rule(sqt, [-8, -8, -8], [16, 16, 16], [4], 0.5, 1.0).tolist() == [0]
    # a masked-out pixel stays out whatever its statistics say
    assert _rule(sqt, [[100, 0, 0], [100, 0, 0]], [[10000, 0, 0]] * 2, [8, 8], 0.5, 1.0, mask=[0, 5]).tolist() == [0, 1]


def test_rule_restatement_rounds_every_operation_to_float32(sqt):
    """n * q and s * s are rounded before they are subtracted: with s = 4097 (s * s = 16785409 needs 25 bits and rounds to
    16785408) and q = 16785409 / 2 stored as float32, float64 arithmetic and float32 arithmetic disagree about the sign of L."""
    s = np.float32(4097.0)
    q = np.float32(8392704.0)            # n * q = 16785408 exactly = fl(s * s): L = 0 in float32, -1 in exact arithmetic
    assert float(s) * float(s) == 16785409.0 and np.float32(s * s) == np.float32(16785408.0)
    # eps = 0, tol = 0: converged iff L <= 0
    assert _rule(sqt, [s, 0, 0], [q, 0, 0], [2], 0.0, 0.0).tolist() == [0]
    q_up = np.nextafter(q, np.float32(np.inf))
    assert _rule(sqt, [s, 0, 0], [q_up, 0, 0], [2], 0.0, 0.0).tolist() == [1]
