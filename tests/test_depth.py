"""Caller-given path depth (sq_scene_set_depth), the part that needs no GPU: the C-ABI's declarations, exports and NULL refusals, the
Python wrappers' and the CLIs' refusals, and the expected values of tests/test_gpu_depth.py -- the restatement of depth D in
tests/depth_restatement.py is pinned to the oracle at D = 3, and its inputs are shown to tell depths apart."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import depth_restatement as DR
from bitcmp import ibits, nan_eq
from conftest import DATA, ROOT
from ray_oracle import oracle_raytrace

f32 = np.float32


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_depth_calls(sqt):
    header = open(os.path.join(ROOT, "include", "squigly_hip.h")).read()
    assert re.search(r"\bint\s+sq_scene_set_depth\(sq_device_scene\* s, int32_t depth\);", header)
    assert re.search(r"\bint32_t\s+sq_scene_get_depth\(sq_device_scene\* s\);", header)
    assert '"deep"' in header and "HOST WAIT" in header[header.index("sq_scene_set_lights(sq_device_scene* s,"):header.index("sq_scene_set_depth(")]
    L = sqt.lib()
    for name in ("sq_scene_set_depth", "sq_scene_get_depth"):
        assert getattr(L, name) is not None
        assert name in importlib.import_module("squigly-trace_amd._native").EXPORTED_SYMBOLS
    assert L.sq_abi_version() == 1
    assert re.search(r"#define\s+SQ_ABI_VERSION\s+1\b", header)


def test_null_scene_is_refused_with_a_message(sqt):
    L = sqt.lib()
    assert L.sq_scene_set_depth(None, 3) != 0
    assert b"null" in L.sq_last_error()
    L.sq_scene_get_lights(None, None, 0)                                # another message in between
    assert L.sq_scene_get_depth(None) == -1
    assert len(L.sq_last_error()) > 0


# ---- Python ------------------------------------------------------------------------------------------------------------------
BAD_DEPTHS = (0, 9, -1, 3.0, 2.5, "3", None, True, [3])


@pytest.mark.parametrize("bad", BAD_DEPTHS, ids=repr)
def test_python_wrappers_refuse_a_bad_depth_before_any_device_work(sqt, bad):
    N = importlib.import_module("squigly-trace_amd._native")
    device = importlib.import_module("squigly-trace_amd.device")
    with pytest.raises(sqt.SquiglyError, match="depth"):
        N.depth_value(bad)
    ds = device.DeviceScene.__new__(device.DeviceScene)                  # no upload: a handle that no library call may see
    ds._h = None
    with pytest.raises(sqt.SquiglyError, match="depth"):
        ds.set_depth(bad)
    if bad is None:                                                     # depth=None is "the reference's" in the render functions
        return
    cam = sqt.load_camera(os.path.join(DATA, "camera"))
    with pytest.raises(sqt.SquiglyError, match="depth"):                # bih = None: anything past the check would fail otherwise
        next(sqt.render_progressive(None, cam, 2, (4, 4), 1, depth=bad))
    with pytest.raises(sqt.SquiglyError, match="depth"):
        next(sqt.render_adaptive(None, cam, 2, (4, 4), 0.1, depth=bad))
    with pytest.raises(sqt.SquiglyError, match="depth"):
        sqt.render_views_rgb8(None, [cam], 2, (4, 4), depth=bad)


def test_good_depths_are_taken():
    N = importlib.import_module("squigly-trace_amd._native")
    assert [N.depth_value(d) for d in (1, 3, 8, np.int32(5), np.int64(8))] == [1, 3, 8, 5, 8]
    assert N.MAX_DEPTH == DR.MAX_DEPTH == 8


# ---- the CLIs ----------------------------------------------------------------------------------------------------------------
def test_python_cli_refuses_depth_9_and_depth_with_cast(capsys):
    cli = importlib.import_module("squigly-trace_amd.cli")
    for argv, word in ((["--depth", "9"], "1..8"), (["--depth", "0"], "1..8"), (["--depth", "x"], "1..8"),
                       (["--depth", "4", "--cast"], "--cast")):
        with pytest.raises(SystemExit) as e:
            cli.parse_args(argv)
        assert e.value.code == 2
        assert word in capsys.readouterr().err
    assert cli.parse_args(["--depth", "8"]).depth == 8 and cli.parse_args([]).depth is None


def test_cpp_cli_refuses_depth_9_and_depth_with_cast(sqt):
    exe = os.path.join(os.path.dirname(sqt.LIB_PATH), "bin", "squigly-trace")
    assert os.path.exists(exe), "the C++ CLI is built by build()"
    for argv, word in ((["--depth", "9"], "1..8"), (["--depth=0"], "1..8"), (["--depth", "3x"], "1..8"), (["--depth", "4", "--cast"], "--cast")):
        r = subprocess.run([exe] + argv + ["--objpath", "/nonexistent.obj"], capture_output=True, text=True, cwd=ROOT)
        assert r.returncode == 2, (argv, r.returncode, r.stderr)
        assert "--depth" in r.stderr and word in r.stderr and "Rendering" not in r.stdout, (argv, r.stderr)
    assert "--depth" in subprocess.run([exe, "--help"], capture_output=True, text=True).stdout


# ---- the restatement, pinned to the oracle at D = 3 --------------------------------------------------------------------------
@pytest.mark.parametrize("which", ("bright", "shipped"))
def test_restatement_at_depth_3_is_the_oracles_sample_radiance_on_the_gpu_tests_rays(O, which):
    c = DR.case(which)
    assert len(c.o) == 4 * DR.N_RAYS
    s = c.s.reshape(4, -1)
    assert ((s >= 0) & (s < 1 << 20)).any() and (s >= 1 << 40).any() and (s < 0).any()      # small, huge and negative seeds
    want = oracle_raytrace(O, c.ob, c.o, c.d, c.s)
    got = DR.radiances(DR.case_paths(c), 3)
    ok = nan_eq(got, want).all(-1)
    assert ok.all(), (int((~ok).sum()), np.nonzero(~ok)[0][:8])
    assert (want != 0).any(-1).mean() > (0.3 if which == "bright" else 0.01)
    want1 = oracle_raytrace(O, c.ob, c.o[:300], c.d[:300], c.s[:300], k=1)                  # ... and of the next generator
    assert nan_eq(DR.radiances(DR.paths(c.ob, c.flat, c.o[:300], c.d[:300], c.s[:300], k=1), 3), want1).all()


@pytest.mark.parametrize("which", ("bright", "shipped"))
def test_restatement_at_depth_3_is_the_oracles_render_of_the_16x24_frame(O, which):
    c = DR.case(which)
    cam = O.load_camera(os.path.join(DATA, "camera"))
    avg, rgb, _ = c.ob.render(cam, 3, 16, 24)
    _, _, got = DR.fold_frame(DR.frame_case(which, "camera", 16, 24, 3), 3)
    assert np.array_equal(ibits(got.reshape(16, 24, 3)), ibits(avg)) and avg.any()
    assert np.array_equal(np.array([O.tonemap(a) for a in got], np.uint8).reshape(16, 24, 3), rgb)


# ---- the inputs tell depths apart, judged by the restatement alone -----------------------------------------------------------
def test_the_bright_free_rays_change_with_every_depth_step():
    """At least 0.25 of the free rays (all of them: the family holds rays whose ray 0 hits, depth_restatement.Case) change bits between
    the depths of each pair."""
    c = DR.case("bright")
    trails = DR.case_paths(c)[:DR.N_RAYS]                               # the "free" family comes first
    assert c.families[0] == "free" and len(trails) == DR.N_RAYS and all(t[0] is not None for t in trails)
    shares = {}
    for a, b in ((1, 2), (2, 3), (3, 4), (4, 5), (5, 8)):
        shares[(a, b)] = float((ibits(DR.radiances(trails, a)) != ibits(DR.radiances(trails, b))).any(-1).mean())
    print("bright free rays, share that changes bits between depths:", shares)
    assert min(shares.values()) >= 0.25, shares


def test_the_bright_frame_changes_between_depth_3_and_6():
    fp = DR.frame_case("bright", "camera", 16, 24, 3)
    a, b = DR.fold_frame(fp, 3)[2], DR.fold_frame(fp, 6)[2]
    share = float((ibits(a) != ibits(b)).any(-1).mean())
    print("bright 16 x 24 @ 3, share of pixels that change between depth 3 and 6:", share)
    assert share >= 0.25, share


def test_the_odd_materials_are_odd():
    c = DR.case("odd")
    m = c.otris
    assert np.isinf(m["emissive"]).any() and (m["surf"] < 0).any() and (m["surf"] == 0).all(-1).any()
    r = DR.radiances(DR.case_paths(c), 4)
    assert np.isnan(r).any() and np.isinf(r).any() and (r < 0).any()
