"""Caller-given sky (sq_scene_set_sky), the part that needs no GPU: the C-ABI's declarations, exports and NULL refusals, the Python
wrappers' and the CLIs' refusals, and the expected values of tests/test_gpu_sky.py -- tests/sky_restatement.py is pinned to
tests/depth_restatement.py (and so to the oracle) with no sky, and its inputs are shown to meet the sky at every level."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import depth_restatement as DR
import sky_restatement as SR
from bitcmp import ibits, nan_eq
from conftest import DATA, ROOT
from scenes import ROTATED

f32 = np.float32
DEPTHS = (1, 2, 3, 4, 5, 8)
FRAMES = (("camera", 16, 24), ("camera", 40, 72), ("rotated", 16, 24), ("rotated", 40, 72))


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_sky_calls(sqt):
    header = open(os.path.join(ROOT, "include", "squigly_hip.h")).read()
    assert re.search(r"typedef struct \{ float up\[3\]; float down\[3\]; \} sq_sky;", header)
    assert re.search(r"\bint\s+sq_scene_set_sky\(sq_device_scene\* s, const sq_sky\* sky\);", header)
    assert re.search(r"\bint\s+sq_scene_get_sky\(sq_device_scene\* s, sq_sky\* out\);", header)
    block = header[header.index("sq_scene_get_depth(sq_device_scene* s);"):header.index("sq_scene_set_sky(")]
    for text in ("sky(d_b)", "t = 0.5 * u + 0.5", "sky_c = down_c + t * (up_c - down_c)", "not normalised", "single additions",
                 "sky == NULL", "all +0 is a sky", "s == NULL"):
        assert text in block, text
    L = sqt.lib()
    for name in ("sq_scene_set_sky", "sq_scene_get_sky"):
        assert getattr(L, name) is not None
        assert name in importlib.import_module("squigly-trace_amd._native").EXPORTED_SYMBOLS
    assert L.sq_abi_version() == 1


def test_null_scene_is_refused_with_a_message(sqt):
    L = sqt.lib()
    import ctypes
    sky = (ctypes.c_float * 6)(1, 2, 3, 4, 5, 6)
    assert L.sq_scene_set_sky(None, sky) != 0
    assert b"null" in L.sq_last_error()
    L.sq_scene_get_lights(None, None, 0)                                # another message in between
    assert L.sq_scene_set_sky(None, None) != 0 and b"null" in L.sq_last_error()
    L.sq_scene_get_lights(None, None, 0)
    assert L.sq_scene_get_sky(None, sky) == -1
    assert len(L.sq_last_error()) > 0 and list(sky) == [1, 2, 3, 4, 5, 6]


# ---- Python ------------------------------------------------------------------------------------------------------------------
BAD_SKIES = ((1, 2), (1, 2, 3, 4), "1,2,3", 5.0, [[1, 2, 3]] * 3, object())


# (repr of the bare object() holds its address, which differs from run to run: that case gets a name that stays)
@pytest.mark.parametrize("bad", BAD_SKIES, ids=lambda b: "object()" if type(b) is object else repr(b))
def test_python_wrappers_refuse_a_bad_sky_before_any_device_work(sqt, bad):
    N = importlib.import_module("squigly-trace_amd._native")
    device = importlib.import_module("squigly-trace_amd.device")
    with pytest.raises(sqt.SquiglyError, match="sky"):
        N.sky_value(bad)
    with pytest.raises(sqt.SquiglyError, match="sky"):
        N.sky_value((1, 2, 3), bad)
    ds = device.DeviceScene.__new__(device.DeviceScene)                  # no upload: a handle that no library call may see
    ds._h = None
    with pytest.raises(sqt.SquiglyError, match="sky"):
        ds.set_sky(bad)
    with pytest.raises(sqt.SquiglyError, match="sky"):
        ds.set_sky(None, (1, 2, 3))
    if isinstance(bad, tuple) and len(bad) == 2:                        # sky= reads two items as (up, down): refused for its `up`
        bad = ((1, 2), (1, 2, 3))
    cam = sqt.load_camera(os.path.join(DATA, "camera"))
    with pytest.raises(sqt.SquiglyError, match="sky"):                  # bih = None: anything past the check would fail otherwise
        next(sqt.render_progressive(None, cam, 2, (4, 4), 1, sky=bad))
    with pytest.raises(sqt.SquiglyError, match="sky"):
        next(sqt.render_adaptive(None, cam, 2, (4, 4), 0.1, sky=bad))
    with pytest.raises(sqt.SquiglyError, match="sky"):
        sqt.render_views_rgb8(None, [cam], 2, (4, 4), sky=bad)


def test_good_skies_are_taken_as_they_are():
    N = importlib.import_module("squigly-trace_amd._native")
    a = N.sky_value((1, 2, 3))
    assert a.dtype == f32 and a.shape == (2, 3) and (a[0] == a[1]).all() and list(a[0]) == [1, 2, 3]
    b = N.sky_value(np.array([np.inf, -1, np.nan]), [0.0, -0.0, 7])
    assert np.isinf(b[0, 0]) and b[0, 1] == -1 and np.isnan(b[0, 2]) and np.signbit(b[1, 1]) and b[1, 2] == 7   # values are not checked
    assert N.sky_pair(None) is None
    assert np.array_equal(N.sky_pair((1, 2, 3)), a) and np.array_equal(N.sky_pair(((1, 2, 3), (4, 5, 6)))[1], f32([4, 5, 6]))


# ---- the CLIs ----------------------------------------------------------------------------------------------------------------
def test_python_cli_parses_sky_and_refuses_it_with_cast(capsys):
    cli = importlib.import_module("squigly-trace_amd.cli")
    for argv, word in ((["--sky", "1,2"], "R,G,B"), (["--sky", "1,2,3,4"], "R,G,B"), (["--sky", "a,b,c"], "R,G,B"),
                       (["--sky", "1,2,3", "--cast"], "--cast")):
        with pytest.raises(SystemExit) as e:
            cli.parse_args(argv)
        assert e.value.code == 2
        assert word in capsys.readouterr().err
    assert cli.parse_args([]).sky is None
    assert cli.parse_args(["--sky", "0.25,0.5,1"]).sky == ((0.25, 0.5, 1.0), (0.25, 0.5, 1.0))
    assert cli.parse_args(["--sky=0.25,0.5,1,0.75,0.625,0.5"]).sky == SR.GRADIENT
    assert cli.parse_args(["--sky", "(-1,inf,0,0,0,0)", "--depth", "2"]).sky == ((-1.0, float("inf"), 0.0), (0.0, 0.0, 0.0))


def test_cpp_cli_refuses_a_bad_sky_and_sky_with_cast(sqt):
    exe = os.path.join(os.path.dirname(sqt.LIB_PATH), "bin", "squigly-trace")
    assert os.path.exists(exe), "the C++ CLI is built by build()"
    for argv, word in ((["--sky", "1,2"], "R,G,B"), (["--sky=1,2,3,4"], "R,G,B"), (["--sky", "1,2,3,4,5,6,7"], "R,G,B"), (["--sky", "x"], "R,G,B"),
                       (["--sky", "1,2,3", "--cast"], "--cast")):
        r = subprocess.run([exe] + argv + ["--objpath", "/nonexistent.obj"], capture_output=True, text=True, cwd=ROOT)
        assert r.returncode == 2, (argv, r.returncode, r.stderr)
        assert "--sky" in r.stderr and word in r.stderr and "Rendering" not in r.stdout, (argv, r.stderr)
    # a good sky gets past the parsing: the missing scene is what fails then
    r = subprocess.run([exe, "--sky", "0.25,0.5,1,0.75,0.625,0.5", "--objpath", "/nonexistent.obj"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 1 and "--sky" not in r.stderr, r.stderr
    assert "--sky" in subprocess.run([exe, "--help"], capture_output=True, text=True).stdout


# ---- the formula ------------------------------------------------------------------------------------------------------------
def test_sky_of_a_few_directions_by_hand():
    up, down = f32(SR.GRADIENT[0]), f32(SR.GRADIENT[1])
    assert np.array_equal(SR.sky_of(SR.GRADIENT, (0, 0, 2)), up) and np.array_equal(SR.sky_of(SR.GRADIENT, (0, 0, -0.5)), down)
    assert np.array_equal(SR.sky_of(SR.GRADIENT, (3, -4, 0)), (down + f32(0.5) * (up - down)).astype(f32))      # the horizon, not normalised
    assert np.isnan(SR.sky_of(SR.GRADIENT, (0, 0, 0))).all() and np.isnan(SR.sky_of(((0, 0, 0), (0, 0, 0)), (0, 0, 0))).all()   # d = 0: t is NaN
    for d in ((1, 2, 3), (-7, 0.5, -1e-30), (1e30, 1, 1)):              # a constant sky is `down` for every finite non-zero d
        assert np.array_equal(ibits(SR.sky_of(SR.CONSTANT, d)), ibits(up))
    inf = ((np.inf, 1, 1), (1, 1, 1))
    assert np.isinf(SR.sky_of(inf, (0, 1, 1))[0]) and np.isnan(SR.sky_of(inf, (0, 0, -1))[0])                  # 0 * inf at t = 0
    assert np.isnan(SR.sky_of(((np.inf, 1, 1), (np.inf, 1, 1)), (0, 1, 1))[0])                                 # inf - inf


# ---- the restatement, pinned to depth_restatement (the oracle at D = 3) with no sky ------------------------------------------
@pytest.mark.parametrize("which", ("bright", "shipped"))
def test_with_no_sky_the_restatement_is_depth_restatements_on_the_gpu_tests_rays(which):
    c = DR.case(which)
    trails, plain = SR.case_paths(c), DR.case_paths(c)
    assert len(trails) == len(plain) == 4 * DR.N_RAYS
    for a, b in zip(trails, plain):                                     # the same walk: the same triangles, a Miss where DR says None
        assert len(a) == len(b) and all((x is None) == isinstance(y, SR.Miss) and (x is None or x.tobytes() == y.tobytes()) for x, y in zip(b, a))
    for depth in DEPTHS:
        got, want = SR.radiances(trails, depth, None), DR.radiances(plain, depth)
        assert np.array_equal(ibits(got), ibits(want)) or nan_eq(got, want).all(), (which, depth)
        assert np.array_equal(np.isnan(got), np.isnan(want))


@pytest.mark.parametrize("which", ("bright", "shipped"))
def test_with_no_sky_the_16x24_frame_is_depth_restatements(which):
    for depth in (1, 3, 5):
        got = SR.fold_frame(SR.frame_case(which, "camera", 16, 24, 3), depth, None)
        want = DR.fold_frame(DR.frame_case(which, "camera", 16, 24, 3), depth)
        for g, e in zip(got, want):
            assert np.array_equal(ibits(g), ibits(e)), (which, depth)
        assert want[2].any()


# ---- the inputs meet the sky, judged by the restatement alone ----------------------------------------------------------------
@pytest.mark.parametrize("which", ("bright", "shipped"))
def test_paths_end_on_a_miss_at_every_level(which):
    levels = [SR.miss_level(t) for t in SR.case_paths(DR.case(which))]
    counts = [sum(1 for m in levels if m == b) for b in range(SR.MAX_DEPTH)]
    print(f"{which}: paths that end on a miss at level 0 .. 7:", counts)
    assert min(counts) >= 50, counts


def test_the_sky_changes_the_bright_free_rays_from_depth_2_on():
    """The family holds rays whose ray 0 hits (depth_restatement.Case), so at D = 1 nothing meets the sky: exactly 0 there.  Level 0
    is covered by the other families and by the frames."""
    c = DR.case("bright")
    trails = SR.case_paths(c)[:DR.N_RAYS]
    assert c.families[0] == "free" and all(not isinstance(t[0], SR.Miss) for t in trails)
    shares = {d: float((ibits(SR.radiances(trails, d, SR.GRADIENT)) != ibits(SR.radiances(trails, d, None))).any(-1).mean()) for d in DEPTHS}
    print("bright free rays, share whose bits the sky changes, by depth:", shares)
    assert shares[1] == 0.0
    assert min(shares[d] for d in DEPTHS if d >= 2) >= 0.25, shares


def test_the_gradient_differs_from_the_constant_sky_wherever_the_sky_shows():
    c = DR.case("bright")
    n = DR.N_RAYS
    assert c.families[:3] == ("free", "surface", "to_light")
    trails = SR.case_paths(c)[:3 * n]
    for depth in DEPTHS:
        none, grad, const = (ibits(SR.radiances(trails, depth, sky)) for sky in (None, SR.GRADIENT, SR.CONSTANT))
        shows = (grad != none).any(-1)
        assert ((grad != const).any(-1) | ~shows).all(), (depth, int((shows & ~(grad != const).any(-1)).sum()))
        for f in range(3):
            assert depth == 1 or shows[f * n:(f + 1) * n].sum() >= 50, (depth, f)     # (at D = 1 only a ray 0 that misses shows the sky)


@pytest.mark.parametrize("which", ("bright", "shipped"))
def test_absorbing_hits_stand_above_sky_misses(which):
    trails = SR.case_paths(DR.case(which))
    counts = {d: sum(1 for t in trails if SR.absorbing_above_miss(t, d)) for d in (3, 5)}
    print(f"{which}: rays with an absorbing hit above a sky miss at depth 3 and 5:", counts)
    assert min(counts.values()) >= 10, counts


@pytest.mark.parametrize("cam_name, w, h", FRAMES)
def test_the_bright_frames_have_hit_pixels_and_miss_pixels(O, cam_name, w, h):
    c = DR.case("bright")
    cam = O.camera_from_text(open(os.path.join(DATA, "camera"), "rb").read() if cam_name == "camera" else ROTATED)
    hits = np.array([c.ob.intersect(*O.make_ray(w, h, y, x, cam)).hit for y in range(w) for x in range(h)], bool)
    print(f"bright {w} x {h}, {cam_name}: {int((~hits).sum())} of {w * h} primary rays miss")
    assert hits.sum() >= 20 and (~hits).sum() >= 20


# ---- random scenes ----------------------------------------------------------------------------------------------------------
FUZZ_SEEDS = range(1000, 1100)


class Row:
    pass


@pytest.fixture(scope="module")
def fuzz_table(sqt, O):
    import fuzz_features as FF
    out = []
    for seed in FUZZ_SEEDS:
        c = FF.case(seed)
        sky = SR.fuzz_sky(seed)
        r = Row()
        r.seed = seed
        fp, rp = SR.fuzz_frame_paths(c), SR.fuzz_ray_paths(c)
        prim = [isinstance(t[0], SR.Miss) for t in fp[0]]
        r.hit_and_miss = any(prim) and not all(prim)
        r.sky_changes = bool((FF.canon(SR.radiances(rp, c.depth, sky)) != FF.canon(SR.radiances(rp, c.depth, None))).any())
        every = rp + [t for trails in fp for t in trails]
        r.deep_miss = any((SR.miss_level(t, c.depth) or 0) >= 2 for t in every)
        r.absorbing = any(SR.absorbing_above_miss(t, c.depth) for t in every)
        # the pin, on every seed: with no sky the frame and the batch are depth_restatement's
        same_frame = all(np.array_equal(FF.canon(g.reshape(e.shape)), FF.canon(e))
                         for g, e in zip(SR.fold_frame(fp, c.depth, None), FF.deep_frame(c, c.depth)[:3]))
        r.pin = same_frame and np.array_equal(FF.canon(SR.radiances(rp, c.depth, None)), FF.canon(FF.DR.radiances(FF.ray_paths(c), c.depth)))
        out.append(r)
    return out


def test_with_no_sky_every_random_scene_is_depth_restatements(fuzz_table):
    assert [r.seed for r in fuzz_table if not r.pin] == []


FUZZ_COVERAGE = (
    ("the frame has both a primary hit and a primary miss", lambda r: r.hit_and_miss, 30),
    ("the sky changes a ray of the batch at the drawn depth", lambda r: r.sky_changes, 95),
    ("a path misses at level 2 or deeper, inside the depth", lambda r: r.deep_miss, 25),
    ("an absorbing hit stands above a sky miss", lambda r: r.absorbing, 15),
)


@pytest.mark.parametrize("what, fact, least", FUZZ_COVERAGE, ids=[c[0] for c in FUZZ_COVERAGE])
def test_the_random_scenes_cover(fuzz_table, what, fact, least):
    count = sum(1 for r in fuzz_table if fact(r))
    print(f"seeds {FUZZ_SEEDS[0]}..{FUZZ_SEEDS[-1]} where {what}: {count} (at least {least} asked)")
    assert count >= least, f"{what}: {count} seeds, {least} asked"
