"""Moving geometry and the history clamp without a GPU: sq_temporal_accumulate_moving_device's surface and refusals, the numpy
restatement of its contract (tests/moving_restatement.py) against the old contract's and against csrc/sq_temporal_pixel.h compiled as a
program of its own (plainly and under the sanitizers), the clamp's properties, and the host helpers (back_transforms, moved_mesh)."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import library_surface as LS
import moving_restatement as M
import temporal_restatement as R
from bitcmp import same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NO_DEVICE = 1 << 20         # a device number no machine has: a call the checks let through by mistake fails there, before any launch
CAM = ((0, 0, 0), R.IDENTITY)
PREV_CAM = ((0.3, 0.03, -0.02), R.turned(0.01))
SIGMA_P = 0.05


@pytest.fixture(scope="module")
def tp(sqt):
    mod = importlib.import_module("squigly-trace_amd.temporal")
    mod.lib()
    return mod


def test_the_new_entry_point_is_exported(tp):
    declared = LS.check_exports(tp, "squigly_temporal.h", "sq_temporal_")
    assert "sq_temporal_accumulate_moving_device" in declared and "sq_temporal_accumulate_moving_device" in tp.EXPORTED_SYMBOLS
    LS.check_client(tp.LIB_PATH, False)


# ---- the restatement against the old contract's ----
@pytest.mark.parametrize("rows, cols, seed", [(1, 1, 1), (5, 7, 2), (17, 67, 3), (48, 64, 4)])
def test_nothing_moving_is_the_old_contract(rows, cols, seed):
    """No objects and no clamp, and a table in which everything is static with tri on both sides of n_tris: temporal_restatement's
    bits, on frames with NaN and infinite colours, with and without alpha and history."""
    cur, prev = R.synthetic(rows, cols, seed, CAM, 0.01), R.synthetic(rows, cols, seed + 10, PREV_CAM, 0.01)
    assert rows * cols < 100 or (np.isnan(cur[0]).any() and np.isinf(cur[0]).any())
    alpha = np.random.default_rng(seed).random((rows, cols)).astype(f32)
    static = np.full(15, -1, np.int32)                       # triangle 10 is inside the table, triangle 20 beyond it
    back = np.full((2, 12), np.nan, f32)                     # never read: no index is in 0..1
    for pb, pc in ((None, None), (R.first_block(*prev), PREV_CAM)):
        for a in (None, alpha):
            want = R.accumulate(*cur, pc, pb, alpha=a, sigma_p=SIGMA_P)
            for kw in (dict(), dict(objects=static, back=back)):
                got = M.accumulate(*cur, pc, pb, alpha=a, sigma_p=SIGMA_P, **kw)
                assert same(got["color"], want["color"]) and same(got["var"], want["var"]) and np.array_equal(got["len"], want["len"])
                for name in R.BLOCK_FIELDS:
                    assert same(got["block"][name].view(f32) if got["block"][name].dtype != f32 else got["block"][name],
                                want["block"][name].view(f32) if want["block"][name].dtype != f32 else want["block"][name]), name
                assert not (got["flags"] & (M.CLAMPED | M.MOVED)).any()
                assert np.array_equal((got["flags"] & M.BLENDED) != 0, want["len"] > 1)         # (max_history > 1: a blend is len >= 2)
    if rows * cols > 30:
        assert (want["len"] == 2).any()


def test_objects_take_history_the_old_contract_rejects():
    """The far wall slides 0.05 along y between two frames of a still camera: reprojected through its back transform every wall
    pixel finds the surface point it shows (len 2, flagged MOVED | BLENDED); without it the plane stop still accepts the taps, but
    they are another surface point's: the wrong history."""
    rows, cols = 24, 32
    cur = R.synthetic(rows, cols, 5, CAM, 0.0, background=0.0)
    prev = R.synthetic(rows, cols, 6, CAM, 0.0, background=0.0)
    objects, back = M.tables(32, 7)
    objects[R.FAR_TRI], objects[R.NEAR_TRI] = 4, -1         # row 4: the sideways slide; the strip in front is static
    pb = R.first_block(*prev)
    moved = M.accumulate(*cur, CAM, pb, objects=objects, back=back, sigma_p=SIGMA_P)
    plain = R.accumulate(*cur, CAM, pb, sigma_p=SIGMA_P)
    wall = cur[2] == R.FAR_TRI
    assert ((moved["flags"][wall] & M.MOVED) != 0).all() and not (moved["flags"][~wall] & M.MOVED).any()
    inner = wall & (np.arange(cols)[None, :] > 2) & (np.arange(cols)[None, :] < cols - 2)
    assert (moved["len"][inner] == 2).all()
    ok = inner & np.isfinite(moved["color"]).all(-1) & np.isfinite(plain["color"]).all(-1)
    assert not same(moved["color"][ok], plain["color"][ok])


# ---- refusals: nothing here reaches a device, the pointers are numbers that are never followed ----
NAMES = ("color", "var", "tri", "normal", "point", "alpha", "prev", "next", "out", "out_var", "out_len", "object", "back", "flags")
BUF = {name: 0x10000000 + i * 0x100000 for i, name in enumerate(NAMES)}
BLOCK = 6 * 5 * 48
nan = float("nan")


def call(tp, sqt, rows=6, cols=5, n_tris=40, n_objects=3, clamp=(1, 1.0), form=0, null_cam=False, params=None, **ptr):
    p = dict(alpha_min=0.1, max_history=32, sigma_p=0.05, cos_n=0.9)
    p.update(params or {})
    P = tp.Params(p["alpha_min"], p["max_history"], p["sigma_p"], p["cos_n"])
    a = {**BUF, **ptr}
    cam = sqt.Camera()
    cl = None if clamp is None else tp.Clamp(*clamp)
    rc = tp.lib().sq_temporal_accumulate_moving_device(
        NO_DEVICE, rows, cols, a["color"], a["var"], a["tri"], a["normal"], a["point"], a["alpha"], None if null_cam else C.byref(cam),
        a["prev"], C.byref(P), a["object"], n_tris, a["back"], n_objects, None if cl is None else C.byref(cl), form, a["next"], a["out"],
        a["out_var"], a["out_len"], a["flags"], None)
    return rc, tp.lib().sq_temporal_last_error().decode()


REFUSALS = [
    # what the old entry point refuses
    (dict(color=None), "null argument"), (dict(next=None), "null argument"), (dict(null_cam=True), "prev_cam is required"),
    (dict(rows=0), "at least 1"), (dict(rows=46341, cols=46341), "exceed 2\\^31 - 1"), (dict(params={"alpha_min": nan}), "alpha_min"),
    (dict(params={"max_history": 0}), "max_history"), (dict(params={"sigma_p": -1.0}), "sigma_p"), (dict(params={"cos_n": nan}), "cos_n"),
    (dict(prev=BUF["prev"] + 4), "d_prev must be 16-byte aligned"), (dict(next=BUF["prev"]), "d_prev and d_next overlap"),
    (dict(out=BUF["normal"]), "d_normal and d_out overlap"),
    # the new ones
    (dict(n_tris=-1), "must not be negative"), (dict(n_objects=-1), "must not be negative"),
    (dict(n_tris=-1, object=None, back=None), "must not be negative"),
    (dict(object=None), "go together"), (dict(back=None), "go together"),
    (dict(n_tris=0), "n_tris = 0"), (dict(n_objects=0), "n_objects = 0"),
    (dict(clamp=(0, 1.0)), "radius"), (dict(clamp=(4, 1.0)), "radius"), (dict(clamp=(-1, 1.0)), "radius"),
    (dict(clamp=(1, -0.5)), "clamp.k"), (dict(clamp=(1, nan)), "clamp.k"),
    (dict(form=-1), "form"), (dict(form=3), "form"),
    (dict(out=BUF["color"]), "d_color and d_out overlap"),                      # allowed without a clamp, refused under one
    (dict(object=BUF["tri"]), "d_tri and d_object overlap"), (dict(back=BUF["color"] + 4), "d_color and d_back overlap"),
    (dict(object=BUF["next"] + 16), "d_next and d_object overlap"), (dict(back=BUF["object"] + 4 * 39), "d_object and d_back overlap"),
    (dict(flags=BUF["out_len"] + 4 * 29), "d_out_len and d_out_flags overlap"), (dict(flags=BUF["out"]), "d_out and d_out_flags overlap"),
    (dict(flags=BUF["back"] + 48 * 3 - 1), "d_back and d_out_flags overlap"), (dict(flags=BUF["prev"]), "d_prev and d_out_flags overlap"),
]


@pytest.mark.parametrize("kw, message", REFUSALS, ids=[f"{i:02d}-{m[:12]}" for i, (_, m) in enumerate(REFUSALS)])
def test_refusals_need_no_gpu(tp, sqt, kw, message):
    rc, err = call(tp, sqt, **kw)
    assert rc != 0 and re.search(message, err), err


def test_what_is_allowed_gets_past_the_checks(tp, sqt):
    """Every optional argument alone and together, d_out_var == d_var under a clamp, d_out == d_color without one, tables that end
    where the next buffer begins, the extreme clamps and every form pass every check: on a device that does not exist the call
    fails at its first runtime call, and with that call's message."""
    for kw in (dict(), dict(object=None, back=None), dict(clamp=None), dict(flags=None), dict(object=None, back=None, clamp=None, flags=None),
               dict(object=None, back=None, n_tris=0, n_objects=0), dict(out_var=BUF["var"]), dict(clamp=None, out=BUF["color"]),
               dict(prev=None, null_cam=True), dict(clamp=(3, 0.0)), dict(clamp=(1, float("inf"))), dict(form=1), dict(form=2),
               dict(back=BUF["object"] + 4 * 40), dict(flags=BUF["back"] + 48 * 3), dict(n_tris=2 ** 31 - 1, object=1 << 40),
               dict(n_objects=2 ** 31 - 1, back=1 << 42)):
        rc, err = call(tp, sqt, **kw)
        assert rc != 0 and "hipSetDevice" in err, (kw, err)


def test_python_refusals(tp, sqt, product_scene):
    for bad in (-1.0, nan, "1", True, (1.0, 0), (1.0, 4), (1.0, 2.0), (1.0, 1, 1)):
        with pytest.raises(ValueError, match="clamp|radius"):
            tp.clamp_arg(bad)
    assert tp.clamp_arg(None) is None and tp.clamp_arg(2) == (2.0, 1) and tp.clamp_arg((0.5, 3)) == (0.5, 3)
    assert tp.clamp_arg(float("inf")) == (float("inf"), 1)
    with pytest.raises(ValueError, match="clamp"):
        sqt.Temporal(None, 48, 64, 16, clamp=-1)
    with pytest.raises(ValueError, match="poses must be"):
        tp.back_transforms(np.zeros((2, 3, 4)), np.zeros((3, 3, 4)))
    with pytest.raises(ValueError, match="poses must be"):
        tp.back_transforms(np.zeros((2, 12)), np.zeros((2, 12)))
    mesh = product_scene[2]
    with pytest.raises(ValueError, match="a pose per material"):
        sqt.moved_mesh(mesh, np.zeros((len(mesh.materials) + 1, 3, 4)))
    render = importlib.import_module("squigly-trace_amd.render")
    still = np.tile(np.eye(3, 4), (1, len(mesh.materials), 1, 1))
    for args, kw, message in (((mesh, [], still, 4, (48, 64)), {}, "at least one camera"),
                              ((mesh, [sqt.Camera()] * 2, still, 4, (48, 64)), {}, "poses must have shape"),
                              ((mesh, [sqt.Camera()], still, 0, (48, 64)), {}, "spp"),
                              ((mesh, [sqt.Camera()], still, 4, (48, 64)), dict(clamp=(1.0, 9)), "radius"),
                              ((mesh, [sqt.Camera()], still, 4, (48, 64)), dict(build="gpu"), "build must be")):
        with pytest.raises(ValueError, match=message):
            next(render.render_moving_sequence(*args, **kw))


def test_cli_flags(sqt, tmp_path):
    import temporal_room as TR
    cli = importlib.import_module("squigly-trace_amd.cli")
    seq = tmp_path / "move.cams"
    seq.write_text("".join(t.decode() for t in TR.CAMERA_TEXTS[:3]))
    poses = tmp_path / "poses.npy"
    np.save(poses, np.tile(np.eye(3, 4), (3, 5, 1, 1)))
    a = cli.parse_args(["--sequence", str(seq), "--temporal", "--poses", str(poses), "--history-clamp", "1.5,2"])
    assert a.poses.shape == (3, 5, 3, 4) and a.history_clamp == (1.5, 2)
    assert cli.parse_args(["--sequence", str(seq), "--temporal", "--history-clamp", "2"]).history_clamp == (2.0, 1)
    assert cli.parse_args(["--sequence", str(seq), "--temporal"]).poses is None
    short, pickled, flat = tmp_path / "short.npy", tmp_path / "pickled.npy", tmp_path / "flat.npy"
    np.save(short, np.tile(np.eye(3, 4), (2, 5, 1, 1)))
    np.save(pickled, np.array([{"a": 1}], dtype=object), allow_pickle=True)
    np.save(flat, np.zeros((3, 5, 12)))
    for bad in (["--poses", str(poses)], ["--sequence", str(seq), "--poses", str(poses)], ["--sequence", str(seq), "--history-clamp", "1"],
                ["--sequence", str(seq), "--temporal", "--poses", str(short)], ["--sequence", str(seq), "--temporal", "--poses", str(pickled)],
                ["--sequence", str(seq), "--temporal", "--poses", str(flat)], ["--sequence", str(seq), "--temporal", "--poses", str(tmp_path / "none.npy")],
                ["--sequence", str(seq), "--temporal", "--poses", str(poses), "--sparse", "2"],
                ["--sequence", str(seq), "--temporal", "--history-clamp", "-1"], ["--sequence", str(seq), "--temporal", "--history-clamp", "1,4"],
                ["--sequence", str(seq), "--temporal", "--history-clamp", "nan"], ["--sequence", str(seq), "--temporal", "--history-clamp", "1,2,3"]):
        with pytest.raises(SystemExit):
            cli.parse_args(bad)


# ---- csrc/sq_temporal_pixel.h as a program of its own ----
def pack(path, cur, prev_cam, prev, alpha, objects, back, clamp, params):
    rows, cols = cur[2].shape
    head = np.array([rows, cols, prev is not None, alpha is not None, -1 if objects is None else len(objects),
                     0 if back is None else len(back), 0 if clamp is None else clamp[0], params["max_history"]], np.int32)
    pos, rot = R.camera(prev_cam if prev_cam is not None else CAM)
    fl = np.concatenate([np.array([0 if clamp is None else clamp[1], params["alpha_min"], params["sigma_p"], params["cos_n"]], f32), pos, rot])
    parts = [head, fl.astype(f32), cur[0], cur[1], cur[2].astype(np.int32), cur[3], cur[4]]
    if alpha is not None:
        parts.append(alpha)
    if prev is not None:
        parts += [prev[k] for k in R.BLOCK_FIELDS]
    if objects is not None:
        parts += [objects.astype(np.int32), back.astype(f32)]
    with open(path, "wb") as fh:
        for p in parts:
            fh.write(np.ascontiguousarray(p).tobytes())


def unpack(path, rows, cols):
    n = rows * cols
    w = np.fromfile(path, np.uint32)
    assert len(w) == 6 * n
    return dict(color=w[:3 * n].view(f32).reshape(rows, cols, 3), var=w[3 * n:4 * n].view(f32).reshape(rows, cols),
                len=w[4 * n:5 * n].view(np.int32).reshape(rows, cols), flags=w[5 * n:].view(np.int32).reshape(rows, cols).astype(np.uint8))


def main_cases():
    """(label, cur, prev_cam, prev block, alpha, objects, back, clamp, params): 5 x 7, where the widest window is larger than the
    image, and 17 x 67; every kind of object index and transform row, tri on both sides of n_tris; every radius; k 0, 1, +inf."""
    inf = float("inf")
    params = dict(R.DEFAULTS, sigma_p=SIGMA_P)
    for rows, cols in ((5, 7), (17, 67)):
        cur, prev = R.synthetic(rows, cols, 21, CAM, 0.01), R.synthetic(rows, cols, 22, PREV_CAM, 0.01)
        M.scatter_triangles(cur[2], 40, 25)                # ids on both sides of every n_tris below
        cur[2][0, 0] = 2 ** 31 - 1
        cur[2][rows - 1, cols - 1] = 14
        alpha = np.random.default_rng(23).random((rows, cols)).astype(f32)
        pb = R.first_block(*prev)
        for n_tris in (15, 21, 40):                       # triangle 20 is beyond the table, its last entry, inside it
            objects, back = M.tables(n_tris, 24 + n_tris)
            for clamp in (None, (1, 0.0), (2, 1.0), (3, inf), (3, 1.0)):
                yield (f"{rows}x{cols}-t{n_tris}-c{clamp}", cur, PREV_CAM, pb, alpha, objects, back, clamp, params)
        yield (f"{rows}x{cols}-first", cur, None, None, None, objects, back, (1, 1.0), params)
        yield (f"{rows}x{cols}-plain", cur, PREV_CAM, pb, None, None, None, None, params)


def static_cases():
    """(label, cur, prev_cam, prev block, alpha, params): what the old entry point takes -- no tables, no clamp -- on the same two
    frames (NaN and infinite colours among them), with and without a previous block and alpha."""
    params = dict(R.DEFAULTS, sigma_p=SIGMA_P)
    for rows, cols in ((5, 7), (17, 67)):
        cur, prev = R.synthetic(rows, cols, 21, CAM, 0.01), R.synthetic(rows, cols, 22, PREV_CAM, 0.01)
        alpha = np.random.default_rng(23).random((rows, cols)).astype(f32)
        for pcam, pb in ((None, None), (PREV_CAM, R.first_block(*prev))):
            for a in (None, alpha):
                yield (f"{rows}x{cols}-static-prev{pb is not None}-alpha{a is not None}", cur, pcam, pb, a, params)


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "asan-ubsan"])
def test_the_pixel_header_as_a_program(tmp_path, sanitized):
    """tests/moving_main.cpp (its own main over csrc/sq_temporal_pixel.h, the text the kernel compiles) built with g++ plainly and
    with -fsanitize=address,undefined, run as a program: exit 0, nothing on stderr, and the restatement's bits.  The static cases
    (no tables, radius 0: what the old entry point runs) are held to the old contract's restatement itself."""
    exe = str(tmp_path / "moving_main")
    flags = ["-fsanitize=address,undefined", "-static-libasan", "-static-libubsan"] if sanitized else ["-O1"]
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off"] + flags + [os.path.join(ROOT, "tests", "moving_main.cpp"), "-o", exe],
                          stderr=subprocess.DEVNULL)
    seen = 0
    for label, cur, pcam, pb, alpha, objects, back, clamp, params in main_cases():
        src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        pack(src, cur, pcam, pb, alpha, objects, back, clamp, params)
        r = subprocess.run([exe, src, dst], capture_output=True)
        assert r.returncode == 0 and r.stderr == b"", (label, r.returncode, r.stderr[-2000:])
        rows, cols = cur[2].shape
        got = unpack(dst, rows, cols)
        want = M.accumulate(*cur, pcam, pb, alpha=alpha, objects=objects, back=back, clamp=clamp, **params)
        assert same(got["color"], want["color"]) and same(got["var"], want["var"]), label
        assert np.array_equal(got["len"], want["len"]) and np.array_equal(got["flags"], want["flags"]), label
        seen |= int(np.bitwise_or.reduce(want["flags"].reshape(-1)))
    assert seen == M.BLENDED | M.CLAMPED | M.MOVED
    blended = 0
    for label, cur, pcam, pb, alpha, params in static_cases():
        src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        pack(src, cur, pcam, pb, alpha, None, None, None, params)
        r = subprocess.run([exe, src, dst], capture_output=True)
        assert r.returncode == 0 and r.stderr == b"", (label, r.returncode, r.stderr[-2000:])
        got = unpack(dst, *cur[2].shape)
        want = R.accumulate(*cur, pcam, pb, alpha=alpha, **params)
        assert same(got["color"], want["color"]) and same(got["var"], want["var"]) and np.array_equal(got["len"], want["len"]), label
        # (max_history > 1: a blend is len >= 2, and without one the frame's own colour comes back)
        assert np.array_equal(got["flags"], np.where(want["len"] > 1, M.BLENDED, 0).astype(np.uint8)), label
        assert same(got["color"][want["len"] == 1], cur[0][want["len"] == 1]), label
        blended += int((want["len"] > 1).sum())
    assert blended > 100


# ---- the clamp's properties, on the restatement ----
def finite_frames(rows, cols, seed):
    """The synthetic frames with finite colours (the properties are orderings of numbers)."""
    out = []
    for s, cam in ((seed, CAM), (seed + 1, PREV_CAM)):
        fr = list(R.synthetic(rows, cols, s, cam, 0.01))
        rng = np.random.default_rng(s)
        fr[0] = rng.gamma(2.0, 1.0, (rows, cols, 3)).astype(f32)
        out.append(tuple(fr))
    return out


@pytest.mark.parametrize("radius, k", [(1, 0.0), (1, 1.0), (2, 0.5), (3, 2.0)])
def test_the_clamped_colour_stays_between_the_bounds_and_the_frame(radius, k):
    cur, prev = finite_frames(24, 40, 31)
    out = M.accumulate(*cur, PREV_CAM, R.first_block(*prev), clamp=(radius, k), sigma_p=SIGMA_P)
    lo, hi, _ = M.window_bounds(cur[0], cur[2], radius, k)
    blended = (out["flags"] & M.BLENDED) != 0
    assert blended.sum() > 300 and ((out["flags"] & M.CLAMPED) != 0).sum() > 20
    c = cur[0]
    assert (out["color"][blended] >= np.minimum(lo, c)[blended]).all() and (out["color"][blended] <= np.maximum(hi, c)[blended]).all()
    assert same(out["color"][~blended], c[~blended])


def test_an_infinite_k_is_no_clamp_where_the_window_varies():
    cur, prev = finite_frames(24, 40, 33)
    pb = R.first_block(*prev)
    free = M.accumulate(*cur, PREV_CAM, pb, sigma_p=SIGMA_P)
    for radius in (1, 2, 3):
        out = M.accumulate(*cur, PREV_CAM, pb, clamp=(radius, float("inf")), sigma_p=SIGMA_P)
        _, _, sd = M.window_bounds(cur[0], cur[2], radius, 1.0)
        varies = (sd > 0).all(-1) & (cur[2] >= 0)
        assert varies.sum() > 300
        assert same(out["color"][varies], free["color"][varies]) and same(out["var"], free["var"]) and np.array_equal(out["len"], free["len"])
        assert not (out["flags"] & M.CLAMPED).any()


def test_a_step_in_the_light_arrives_at_once_under_the_clamp():
    """The guides stay and a region's input colour steps from one constant to another at frame 3: under the clamp (sd = 0, so
    lo = hi = mu = the new constant) the accumulated colour is the new constant from frame 3 on, bit for bit; without the clamp it
    is not there one frame later."""
    rows, cols, radius = 20, 30, 2
    base = R.synthetic(rows, cols, 41, CAM, 0.0, background=0.0)
    region = np.zeros((rows, cols), bool)
    region[4:16, 5:25] = True
    inner = np.zeros((rows, cols), bool)
    inner[4 + radius:16 - radius, 5 + radius:25 - radius] = True               # windows that lie inside the region
    inner &= base[2] >= 0
    assert inner.sum() > 50
    old, new = np.array([0.25, 0.5, 1.0], f32), np.array([2.0, 0.125, 0.75], f32)
    frames = []
    for i in range(6):
        color = np.full((rows, cols, 3), 0.5, f32)
        color[region] = old if i < 3 else new
        frames.append((color, np.full((rows, cols), 0.01, f32)) + base[2:])
    cams = [CAM] * 6
    with_clamp = M.chain(frames, cams, clamp=(radius, 1.0), sigma_p=SIGMA_P)
    without = M.chain(frames, cams, sigma_p=SIGMA_P)
    for i in range(3, 6):
        assert same(with_clamp[i]["color"][inner], np.broadcast_to(new, with_clamp[i]["color"][inner].shape).copy()), i
        assert (with_clamp[i]["len"][inner] == i + 1).all()                    # the length does not shorten where the clamp bites
    assert ((with_clamp[3]["flags"][inner] & M.CLAMPED) != 0).all() and not (with_clamp[2]["flags"][inner] & M.CLAMPED).any()
    assert (np.abs(without[4]["color"][inner] - new) > 0.05).any(-1).all()


# ---- the host helpers ----
def test_back_transforms_take_a_moved_mesh_to_the_one_before(tp, sqt, product_scene):
    """A point of moved_mesh(mesh, poses_f) taken through back_transforms(poses_{f-1}, poses_f) lands on moved_mesh(mesh,
    poses_{f-1}) to float rounding: both are rounded once from float64, so they differ by a few ulps of the coordinates' size."""
    mesh = product_scene[2]
    n = len(mesh.materials)
    rng = np.random.default_rng(51)
    poses = [np.stack([M.rigid(rng.uniform(-1, 1), rng.normal(size=3), rng.uniform(-2, 2, 3)) for _ in range(n)]) for _ in range(2)]
    poses[0][0] = np.eye(3, 4)
    a, b = sqt.moved_mesh(mesh, poses[0]), sqt.moved_mesh(mesh, poses[1])
    rest = mesh.tris
    assert np.array_equal(a.tris["mat"], rest["mat"]) and len(a) == len(mesh)
    still = rest["mat"] == 0
    assert still.any() and all(np.array_equal(a.tris[v][still].view(np.uint32), rest[v][still].view(np.uint32)) for v in ("v0", "v1", "v2"))
    back = tp.back_transforms(poses[0], poses[1])
    assert back.shape == (n, 12) and back.dtype == f32
    B = back.astype(np.float64).reshape(n, 3, 4)[rest["mat"]]
    scale = max(np.abs(a.tris[v]).max() for v in ("v0", "v1", "v2")) + np.abs(poses[1][:, :, 3]).max()
    for v in ("v0", "v1", "v2"):
        p = b.tris[v].astype(np.float64)
        got = np.einsum("nij,nj->ni", B[:, :, :3], p) + B[:, :, 3]
        assert np.abs(got - a.tris[v]).max() <= 16 * np.finfo(f32).eps * scale
    assert same(tp.back_transforms(poses[0], poses[0]), np.tile(M.IDENTITY_ROW, (n, 1))) or \
        np.abs(tp.back_transforms(poses[0], poses[0]) - M.IDENTITY_ROW).max() < 1e-6
