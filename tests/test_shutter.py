"""Motion blur without a GPU: the numpy restatement of include/squigly_shutter.h (tests/shutter_restatement.py) pinned to the
oracle's camera, what the test motion covers, and the surface of libsquigly_shutter.so -- the header, the exports, the ids,
sq_shutter_pose against the restatement (also under the sanitizers, as a program of its own), every refusal that needs no device,
the Python layer's refusals and the CLI's flags."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import lens_restatement as LR
import library_surface as LS
import shutter_restatement as SH
from bitcmp import nan_eq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NO_DEVICE = 1 << 20         # a device number no machine has: a call the checks let through by mistake fails there, before any launch
W, H = SH.W, SH.H
nan, inf = float("nan"), float("inf")


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.fixture(scope="module")
def shutter(sqt):
    mod = importlib.import_module("squigly-trace_amd.shutter")
    mod.lib()
    return mod


@pytest.fixture(scope="module")
def lens(sqt):
    mod = importlib.import_module("squigly-trace_amd.lens")
    mod.lib()
    return mod


@pytest.fixture(scope="module")
def mlens(sqt):
    mod = importlib.import_module("squigly-trace_amd.mlens")
    mod.lib()
    return mod


def raw_motion(shutter, motion=SH.MOTION, time_jitter=1.0):
    """A Motion with unchecked values: the library's own checks are what is under test."""
    m = shutter.Motion.__new__(shutter.Motion)
    f3 = C.c_float * 3
    C.Structure.__init__(m, f3(*motion[0]), f3(*motion[1]), f3(*motion[2]), f3(*motion[3]), time_jitter)
    return m


# ---- (a) the restatement meets the oracle, and the test motion bites ----
def test_the_open_pose_is_the_oracles_camera(O):
    cam = O.load_camera(os.path.join(ROOT, "data", "camera"))
    pos, rot = O.camera_arrays(cam)
    got_pos, got_rot = SH.pose(SH.MOTION, 0.0)
    assert np.array_equal(bits(got_pos), bits(pos)) and np.array_equal(bits(got_rot), bits(rot))
    # a plain sub-ray 0 without time jitter is makeRay's ray under that camera
    for (y, x) in ((0, 0), (7, 13), (W - 1, H - 1)):
        o, d, base, tt = SH.sub_ray(SH.MOTION, 0.0, LR.PLAIN, SH.S, 4, W, H, y, x, 0)
        wo, wd = O.make_ray(W, H, y, x, cam)
        assert tt == 0 and np.array_equal(bits(o), bits(wo)) and np.array_equal(bits(d), bits(wd)) and base == SH.S * (x + y * W)


def test_instants_are_stratified(O):
    """Sub-ray r takes its instant from the r-th of R equal parts of the exposure: its start without time jitter, anywhere in it with."""
    seen = []
    for R in (1, 2, 4, 8):
        for r in range(R):
            assert SH.instant(0.0, SH.S, R, W, 3, 5, r) == f32(r) / f32(R)
            for x in range(H):
                for tj in (0.5, 1.0):
                    tt = SH.instant(tj, SH.S, R, W, 3, x, r)
                    assert f32(r) / f32(R) <= tt <= f32(f32(r) + f32(tj)) / f32(R)
                    if tj == 1.0:
                        seen.append(float(tt) * R - r)
    seen = np.array(seen)
    assert seen.min() < 0.02 and seen.max() > 0.98 and abs(seen.mean() - 0.5) < 0.05           # the draws fill their part
    # m4 is a word of its own: not one of the four the lens draws from
    words = O.tfgen_words(~int(LR.seed_base(SH.S, 4, W, 3, 5, 1)))
    assert words[4] not in words[:4]


def test_the_motion_moves_the_picture():
    """Counted on the CPU oracle at 16 x 24 under the shipped scene: the first-hit triangle differs from tt = 0 on 0.34 / 0.42 / 0.45 /
    0.45 of the pixels at tt = 0.25 / 0.5 / 0.75 / 1, on 0.28 of them between 0.75 and 1, and 118 to 156 of the 384 pixels hit the
    scene at every instant.  Floors of 0.25, 0.2 and 100 keep the GPU comparisons from being vacuous."""
    c, _ = LR.room("shipped")
    tri = {tt: SH.first_hits_at(c.ob, SH.MOTION, tt) for tt in (0.0, 0.25, 0.5, 0.75, 1.0)}
    shares = {tt: float((tri[tt] != tri[0.0]).mean()) for tt in (0.25, 0.5, 0.75, 1.0)}
    late = float((tri[1.0] != tri[0.75]).mean())
    hits = {tt: int((t >= 0).sum()) for tt, t in tri.items()}
    print(f"first hits differing from tt = 0: {shares}; between 0.75 and 1: {late:.3f}; hit pixels: {hits}")
    assert all(s >= 0.25 for s in shares.values()), shares
    assert late >= 0.2
    assert all(n >= 100 for n in hits.values()), hits


# ---- (b) the library's surface ----
def header_text():
    return open(os.path.join(ROOT, "include", "squigly_shutter.h")).read()


def test_header_carries_the_contract():
    text = header_text()
    for line in ("m4   = the fifth output of mkTFGen (NOT base)",
                 "the low half of the third word of the same Threefish block",
                 "tt   = (fromIntegral r + time_jitter * random01 m4) / fromIntegral R",
                 "pos  = pos0 + tt *^ (pos1 - pos0)",
                 "per component: dc = pos1_c - pos0_c ; pos0_c + tt * dc",
                 "ang  = ang0 + tt *^ (ang1 - ang0)",
                 "rot  = rotMatrixRads ang.x ang.y ang.z",
                 "bit for bit what sq_rot_matrix_rads returns for these three floats",
                 "crd sine and cosine, yx = ry * rx, rot = rz * yx, an entry the fold",
                 "r = a[i][k] * b[k][j] + r over k = 0, 1, 2 from r = +0",
                 "o, d = squigly_lens.h's lines with (pos, rot) in place of (pos cam, rotation cam)",
                 "s_r, sum, sum2, count, avg, rgb: squigly_lens.h's (dense) or squigly_mlens.h's (listed), unchanged",
                 "No draw is made when jitter == 0 && aperture == 0 && time_jitter == 0",
                 "float pos0[3], ang0[3];", "float pos1[3], ang1[3];", "float time_jitter;"):
        assert line in text, line
    for word in ("UNCHECKED INPUTS", "SIGNED ZEROS", "-0 + +0 = +0", "INDEX WIDTHS", "2^31 - 1", "HOST WAIT", "Out of scope",
                 "sq_lens_plan", "sq_lens_work_bytes", "sq_lens_fold_device", "sq_mlens_fold_device", "sq_mlens_live_device",
                 "d_count must be", "time_jitter outside [0, 1] or not finite"):
        assert word in text, word


def test_header_functions_are_exported(shutter):
    declared = LS.check_exports(shutter, "squigly_shutter.h", "sq_shutter_")   # (no planner, fold or list export: those stay the lens libraries')
    assert declared == {"sq_shutter_last_error", "sq_shutter_build_id", "sq_shutter_pose", "sq_shutter_rays_device", "sq_shutter_render_device"}


def test_the_other_libraries_did_not_gain_it(sqt, lens, mlens, shutter):
    for h in ("squigly_hip.h", "squigly_host.h", "squigly_denoise.h", "squigly_lens.h", "squigly_mlens.h"):
        assert "sq_shutter" not in open(os.path.join(ROOT, "include", h)).read(), h
    denoise = importlib.import_module("squigly-trace_amd.denoise")
    assert not [s for s in sqt.EXPORTED_SYMBOLS + lens.EXPORTED_SYMBOLS + mlens.EXPORTED_SYMBOLS if "shutter" in s]
    for path in (sqt.LIB_PATH, denoise.LIB_PATH, lens.LIB_PATH, mlens.LIB_PATH):
        assert "sq_shutter" not in subprocess.check_output(["nm", "-D", "--defined-only", path]).decode(), path
    # the two lens libraries export what they exported, and declare what they declared
    assert LS.exported_by(lens.LIB_PATH) == set(lens.EXPORTED_SYMBOLS) == LS.declared_in("squigly_lens.h", "sq_lens_") == {
        "sq_lens_rays_device", "sq_lens_fold_device", "sq_lens_render_device", "sq_lens_plan", "sq_lens_work_bytes", "sq_lens_last_error",
        "sq_lens_build_id"}
    assert LS.exported_by(mlens.LIB_PATH) == set(mlens.EXPORTED_SYMBOLS) == LS.declared_in("squigly_mlens.h", "sq_mlens_") == {
        "sq_mlens_last_error", "sq_mlens_build_id", "sq_mlens_live_device", "sq_mlens_rays_device", "sq_mlens_fold_device",
        "sq_mlens_render_device"}
    b = LS.build_module()
    mine = {"sq_shutter.hip", "sq_shutter_pose.h", "../../include/squigly_shutter.h"}
    assert not mine & set(LS.files(b, "main", "denoise", "lens", "mlens"))
    assert mine | {"sq_lens_plan.h", "sq_lens_ray.h", "sq_lens_frame.h", "../../include/squigly_lens.h"} <= set(LS.files(b, "shutter"))
    sh = b.LIBS["shutter"]
    assert sh["link"] == b.LIBS["lens"]["link"] and sh["salt"] == b"shutter\0" and sh["macro"] == "SQ_SHUTTER_BUILD_ID"
    assert sh["salt"] not in [b.LIBS[n]["salt"] for n in ("lens", "mlens", "main", "denoise")]
    LS.check_client(shutter.LIB_PATH, True, never=("libsquigly_lens", "libsquigly_mlens"))


def test_ids_are_separate(lens, mlens, shutter, sqt, tmp_path):
    b = LS.build_module()
    assert lens.build_id() == b.lib_source_id(b.LIBS["lens"]) and mlens.build_id() == b.lib_source_id(b.LIBS["mlens"])
    own, shared = {"shutter"}, {"lens", "mlens", "shutter"}
    LS.check_ids(b, "shutter", shutter, sqt, tmp_path,
                 [("sq_shutter.hip", own), ("sq_shutter_pose.h", own), ("../../include/squigly_shutter.h", own), ("sq_lens_ray.h", shared),
                  ("sq_lens_frame.h", shared), ("../../include/squigly_mlens.h", {"mlens"})])


# ---- (c) sq_shutter_pose ----
def pose_cases():
    """A few thousand (motion, tt): the test motion, random ones over many magnitudes, and huge, tiny, zero, negative-zero and
    non-finite angles and positions."""
    rng = np.random.default_rng(20)
    cases = [(SH.MOTION, tt) for tt in np.linspace(0, 1, 33)]
    for _ in range(2400):
        scale = 10.0 ** rng.integers(-3, 4)
        m = tuple(tuple(float(v) for v in (rng.standard_normal(3) * scale).astype(f32)) for _ in range(4))
        cases.append((m, float(f32(rng.random()))))
    special = [0.0, -0.0, 1e-30, -1e-38, 1e-45, 3.0e38, -3.0e38, 1e10, 12345.678, inf, -inf, nan, np.pi, -np.pi / 2]
    for i, a in enumerate(special):
        for j, b in enumerate(special):
            ang0, ang1 = (a, 0.25, b), (b, a, -0.5)
            pos0, pos1 = (b, 1.0, a), (2.0, a, b)
            cases.append(((pos0, ang0, pos1, ang1), [0.0, 0.5, 1.0, 0.3][(i + j) % 4]))
    for tt in (-1.0, 2.0, 1e-40, nan, inf):                                    # tt is not checked
        cases.append((SH.MOTION, tt))
    return cases


def test_pose_equals_the_restatement(shutter):
    cases = pose_cases()
    assert len(cases) > 2500
    L = shutter.lib()
    cam = shutter.N.Camera()
    special = 0
    for motion, tt in cases:
        assert L.sq_shutter_pose(C.byref(raw_motion(shutter, motion)), tt, C.byref(cam)) == 0
        pos, rot = SH.pose(motion, tt)
        got = np.array(list(cam.pos) + list(cam.rot), f32)
        want = np.concatenate([pos, rot])
        assert nan_eq(got, want).all(), (motion, tt, got, want)
        special += int(np.isnan(want).any())
    assert special > 50                                                        # the non-finite inputs reach the comparison
    with pytest.raises(shutter.N.SquiglyError, match="null argument"):
        shutter.check(L.sq_shutter_pose(None, 0.0, C.byref(cam)))
    assert L.sq_shutter_pose(C.byref(raw_motion(shutter)), 0.0, None) != 0


def test_equal_poses_give_one_camera(sqt, shutter):
    """With equal poses the camera of every instant is {pos0, sq_rot_matrix_rads(ang0)} -- x + tt * (+0) is x, but for a -0."""
    rng = np.random.default_rng(21)
    L = shutter.lib()
    for i in range(40):
        pos = tuple(float(v) for v in (rng.standard_normal(3) * 10.0 ** rng.integers(-2, 3)).astype(f32))
        ang = tuple(float(v) for v in (rng.standard_normal(3) * 10.0 ** rng.integers(-2, 2)).astype(f32))
        rot = sqt.rot_matrix_rads(*ang).reshape(-1)
        m = raw_motion(shutter, (pos, ang, pos, ang), 0.5)
        for tt in [0.0, 1.0] + [float(f32(t)) for t in rng.random(6)]:
            cam = shutter.N.Camera()
            assert L.sq_shutter_pose(C.byref(m), tt, C.byref(cam)) == 0
            assert np.array_equal(bits(list(cam.pos)), bits(pos)) and np.array_equal(bits(list(cam.rot)), bits(rot)), (pos, ang, tt)
    # SIGNED ZEROS: a -0 component comes out as +0
    cam = shutter.N.Camera()
    L.sq_shutter_pose(C.byref(raw_motion(shutter, ((-0.0, 1.0, -0.0), (0.0, 0.0, 0.0), (-0.0, 1.0, -0.0), (0.0, 0.0, 0.0)))), 0.5, C.byref(cam))
    assert list(bits(list(cam.pos))) == [0, bits([1.0])[0], 0]
    # the Python layer: Motion.pose, from pairs and from camera-file texts
    text = open(os.path.join(ROOT, "data", "camera"), "rb").read()
    shipped = sqt.load_camera(os.path.join(ROOT, "data", "camera"))
    for m in (sqt.Motion(text, text), sqt.Motion(text.decode(), SH.CLOSE), sqt.Motion(SH.OPEN, SH.CLOSE, 0.25)):
        got = m.pose(0)
        assert bytes(got) == bytes(shipped)
    m = sqt.Motion(SH.OPEN, SH.CLOSE)
    assert bytes(m) == bytes(raw_motion(shutter)) and m.time_jitter == 1.0 and "time_jitter=1.0" in repr(m)
    pos, rot = SH.pose(SH.MOTION, 0.5)
    half = m.pose(0.5)
    assert np.array_equal(bits(list(half.pos)), bits(pos)) and np.array_equal(bits(list(half.rot)), bits(rot))
    assert sqt.Motion(SH.OPEN, SH.CLOSE, 0.5).key() != m.key() and sqt.Motion(SH.OPEN, SH.CLOSE).key() == m.key()


def test_pose_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """tests/shutter_pose_main.cpp (its own main over csrc/sq_shutter_pose.h, the host code sq_shutter_pose and the kernels share)
    compiled with -fsanitize=address,undefined and run as a child process, once: exit 0, nothing on stderr, and case by case the
    restatement's pose."""
    exe = str(tmp_path / "shutter_pose_main")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-static-libasan", "-static-libubsan",      # the runtimes inside the program: nothing to order at load time
                           os.path.join(ROOT, "tests", "shutter_pose_main.cpp"), "-o", exe], stderr=subprocess.DEVNULL)
    cases = pose_cases()[::9] + pose_cases()[-60:]
    args = []
    for motion, tt in cases:
        words = bits([v for part in motion for v in part] + [tt])
        args += ["%08x" % int(u) for u in words]
    r = subprocess.run([exe] + args, capture_output=True)
    assert r.returncode == 0 and r.stderr == b"", (r.returncode, r.stderr[-2000:])
    lines = r.stdout.decode().splitlines()
    assert len(lines) == len(cases)
    for line, (motion, tt) in zip(lines, cases):
        got = np.array([int(u, 16) for u in line.split()], np.uint32).view(f32)
        pos, rot = SH.pose(motion, tt)
        assert nan_eq(got, np.concatenate([pos, rot])).all(), (motion, tt, line)


# ---- (d) refusals: nothing here reaches a device, the buffer pointers are numbers that are never followed ----
BUF = {name: 0x10000000 + i * 0x1000000 for i, name in enumerate(("org", "dir", "seed", "index", "sum", "sum2", "count", "avg", "rgb", "work"))}
SCENE = 0x7000000           # stands for a scene: the checks never follow it either
FAR = {name: (i + 1) << 40 for i, name in enumerate(BUF)}


def frame_call(sqt, shutter, lens, which, motion=True, time_jitter=1.0, lens_values=(1.0, 0.0, 1.0), null_lens=False, S=8, R=4, r=(0, 4), w=W,
               h=H, shard=None, listed=False, L=None, work_bytes=None, device=NO_DEVICE, **ptr):
    lib = shutter.lib()
    a = {**BUF, **ptr}
    ln = lens.Lens.__new__(lens.Lens)
    C.Structure.__init__(ln, *lens_values)
    sh = sqt.Shard(*(shard or (w if w > 0 else 1, 0, 1)))
    m = raw_motion(shutter, time_jitter=time_jitter)
    index = a["index"] if listed else None
    n_list = (W * H if L is None else L) if listed else 0
    head = [C.byref(m) if motion else None, None if null_lens else C.byref(ln), S, R, r[0], r[1], w, h, sh, index, n_list]
    if which == "rays":
        rc = lib.sq_shutter_rays_device(device, *head, a["org"], a["dir"], a["seed"], None)
    else:
        wb = lens.work_bytes(W * H, 1) if work_bytes is None else work_bytes
        rc = lib.sq_shutter_render_device(a.get("scene", SCENE), *head, a["work"], wb, a["sum"], a["sum2"], a["count"] if listed else a.get("dense_count"),
                                          a["avg"], a["rgb"], None)
    return rc, lib.sq_shutter_last_error().decode()


FRAME_REFUSALS = [
    (dict(motion=False), "null argument"), (dict(null_lens=True), "null argument"),
    (dict(S=0), "at least 1"), (dict(R=0), "at least 1"), (dict(S=8, R=3), "must divide"), (dict(S=4, R=8, r=(0, 8)), "must divide"),
    (dict(r=(-1, 4)), "bad sub-ray range"), (dict(r=(2, 2)), "bad sub-ray range"), (dict(r=(0, 5)), "bad sub-ray range"),
    (dict(lens_values=(1.5, 0.0, 1.0)), "jitter"), (dict(lens_values=(nan, 0.0, 1.0)), "jitter"),
    (dict(lens_values=(1.0, -0.5, 1.0)), "aperture"), (dict(lens_values=(1.0, inf, 1.0)), "aperture"),
    (dict(lens_values=(1.0, 0.1, 0.0)), "focus"), (dict(lens_values=(1.0, 0.1, nan)), "focus"),
    (dict(time_jitter=-0.1), "time_jitter"), (dict(time_jitter=1.5), "time_jitter"), (dict(time_jitter=nan), "time_jitter"),
    (dict(time_jitter=inf), "time_jitter"), (dict(time_jitter=-inf), "time_jitter"),
    (dict(w=0), "at least 1"), (dict(h=-2), "at least 1"), (dict(shard=(2, 3, 3)), "bad shard"), (dict(shard=(0, 0, 1)), "bad shard"),
    (dict(w=46341, h=46341, work_bytes=1 << 50), r"exceed 2\^31 - 1 pixels"),
    (dict(listed=True, L=-1), "the list must hold"), (dict(listed=True, L=W * H + 1), "the list must hold"),
]
RAYS_REFUSALS = FRAME_REFUSALS + [
    (dict(org=None), "null argument"), (dict(dir=None), "null argument"), (dict(seed=None), "null argument"),
    (dict(w=1024, h=1024, S=4096, R=4096, r=(0, 2048)), r"exceed 2\^31 - 1 ray slots"),
    (dict(w=1024, h=1024, S=4096, R=4096, r=(0, 2048), listed=True, L=2 ** 20), r"exceed 2\^31 - 1 ray slots"),
    (dict(dir=BUF["org"] + 12 * W * H * 4 - 4), "d_org and d_dir overlap"), (dict(seed=BUF["org"]), "d_org and d_seed overlap"),
    (dict(listed=True, index=BUF["org"] + 12), "d_index and d_org overlap"), (dict(listed=True, L=7, dir=BUF["org"] + 12 * 7 * 4 - 4), "d_org and d_dir overlap"),
]
RENDER_REFUSALS = FRAME_REFUSALS + [
    (dict(scene=None), "null argument"), (dict(work=None), "null argument"), (dict(sum=None), "null argument"),
    (dict(dense_count=BUF["count"]), "d_count needs a list"),
    (dict(work_bytes=16895), "too small"), (dict(work_bytes=0), "too small"), (dict(work=BUF["work"] + 8), "16-byte aligned"),
    (dict(listed=True, L=7, work_bytes=44 * 7), "too small"),
    (dict(sum2=BUF["sum"] + 12), "d_sum and d_sum2 overlap"), (dict(rgb=BUF["avg"] + 12 * W * H - 1), "d_avg and d_rgb overlap"),
    (dict(work=BUF["sum"] - 16), "d_sum and d_work overlap"), (dict(listed=True, count=BUF["sum2"]), "d_sum2 and d_count overlap"),
    (dict(listed=True, index=BUF["avg"] + 12), "d_index and d_avg overlap"),
]


@pytest.mark.parametrize("kw, message", RAYS_REFUSALS, ids=[f"{i:02d}-{m[:12]}" for i, (_, m) in enumerate(RAYS_REFUSALS)])
def test_rays_refusals_need_no_gpu(sqt, shutter, lens, kw, message):
    rc, err = frame_call(sqt, shutter, lens, "rays", **kw)
    assert rc != 0 and re.search(message, err), err


@pytest.mark.parametrize("kw, message", RENDER_REFUSALS, ids=[f"{i:02d}-{m[:12]}" for i, (_, m) in enumerate(RENDER_REFUSALS)])
def test_render_refusals_need_no_gpu(sqt, shutter, lens, kw, message):
    rc, err = frame_call(sqt, shutter, lens, "render", **kw)
    assert rc != 0 and re.search(message, err), err


def test_what_is_allowed_gets_past_the_checks(sqt, shutter, lens):
    """Time jitter 0 and 1, the open aperture, a list, the largest batch, no optional buffer: on a device that does not exist they fail
    at the first runtime call, and with its message.  An empty shard and an empty list are no error and touch nothing."""
    for kw in (dict(), dict(time_jitter=0.0), dict(time_jitter=-0.0, lens_values=(0.0, 0.0, nan)), dict(lens_values=(1.0, 0.25, 3.0)),
               dict(listed=True), dict(listed=True, L=1), dict(w=1024, h=1024, S=4096, R=4096, r=(0, 2047), **FAR), dict(r=(3, 4))):
        rc, err = frame_call(sqt, shutter, lens, "rays", **kw)
        assert rc != 0 and "hipSetDevice" in err, err
    for kw in (dict(), dict(sum2=None, avg=None, rgb=None), dict(work_bytes=1 << 20), dict(r=(1, 3)), dict(listed=True), dict(listed=True, count=None)):
        rc, err = frame_call(sqt, shutter, lens, "render", **kw)
        assert rc != 0 and "hipPointerGetAttributes" in err, err
    for which in ("rays", "render"):
        assert frame_call(sqt, shutter, lens, which, w=4, shard=(2, 2, 3))[0] == 0
        assert frame_call(sqt, shutter, lens, which, listed=True, L=0)[0] == 0


# ---- (e) the Python layer ----
def test_python_refusals(sqt, shutter):
    E = sqt.SquiglyError
    for kw, message in ((dict(time_jitter=-0.1), "time_jitter"), (dict(time_jitter=1.01), "time_jitter"), (dict(time_jitter=nan), "time_jitter"),
                        (dict(time_jitter=inf), "time_jitter"), (dict(time_jitter="1"), "time_jitter must be a number"),
                        (dict(time_jitter=True), "time_jitter must be a number"), (dict(time_jitter=None), "time_jitter must be a number")):
        with pytest.raises(E, match=message):
            sqt.Motion(SH.OPEN, SH.CLOSE, **kw)
    for bad in (None, 3, ((0, 0), (0, 0, 0)), ((0, 0, 0),), ((0, 0, "x"), (0, 0, 0)), ((0, 0, 0), (0, 0, 0), (0, 0, 0))):
        with pytest.raises(E, match="open must be"):
            sqt.Motion(bad, SH.CLOSE)
        with pytest.raises(E, match="close must be"):
            sqt.Motion(SH.OPEN, bad)
    with pytest.raises(E):
        sqt.Motion(b"0 7 0.75\n1.57 0", SH.CLOSE)                              # a camera file that is none: the library's own message
    sqt.Motion(((nan, inf, -0.0), (1e30, nan, -inf)), SH.CLOSE, 0)             # positions and angles are not checked
    m, ln = sqt.Motion(SH.OPEN, SH.CLOSE), sqt.Lens()
    unchecked = raw_motion(shutter, time_jitter=2.0)
    # a scene that was never uploaded: whatever gets past its refusal would fail in some other way
    ds = object.__new__(sqt.DeviceScene)
    ds.device, ds._h = 0, None
    cam = sqt.load_camera(os.path.join(ROOT, "data", "camera"))
    for call, message in ((lambda: ds.render_shutter(cam, ln, 8, 4, W, H), "motion must be a Motion"),
                          (lambda: ds.render_shutter(None, ln, 8, 4, W, H), "motion must be a Motion"),
                          (lambda: ds.render_shutter(unchecked, ln, 8, 4, W, H), "time_jitter"),
                          (lambda: ds.render_shutter(m, ln, 8, 3, W, H), "must divide"),
                          (lambda: ds.render_shutter(m, None, 8, 4, W, H), "lens must be a Lens"),
                          (lambda: ds.render_shutter(m, ln, 8, 4, W, H, work_mb=0), "work_mb"),
                          (lambda: ds.render_shutter(m, ln, 8, 4, W, H, shard=(2, 3, 3)), "bad shard"),
                          (lambda: ds.render_shutter(m, ln, 8, 4, W, H, r_range=(2, 4)), "needs the sums"),
                          (lambda: ds.render_shutter(m, ln, 4, 4, 46341, 46341), r"exceed 2\^31 - 1 pixels"),
                          (lambda: ds.shutter_rays(cam, ln, 8, 4, W, H), "motion must be a Motion"),
                          (lambda: ds.shutter_rays(unchecked, ln, 8, 4, W, H), "time_jitter"),
                          (lambda: ds.shutter_rays(m, ln, 8, 4, W, H, r_range=(0, 9)), "bad sub-ray range"),
                          (lambda: ds.shutter_rays(m, ln, 8, 4, W, H, shard=(0, 0, 1)), "bad shard"),
                          (lambda: ds.shutter_rays(m, ln, 4096, 4096, 1024, 1024, r_range=(0, 2048)), r"exceed 2\^31 - 1 ray slots"),
                          (lambda: ds.render_shutter_masked(cam, ln, 8, 4, W, H, 0, 2, None, None, 0), "motion must be a Motion"),
                          (lambda: ds.render_shutter_masked(m, ln, 8, 4, W, H, 2, 2, None, None, 0), "bad sub-ray range"),
                          (lambda: ds.render_shutter_masked(m, ln, 8, 4, W, H, 0, 2, None, None, W * H + 1), "n_live must be"),
                          (lambda: ds.render_shutter_masked(m, ln, 8, 4, W, H, 0, 2, None, None, 4), "needs a sums tensor"),
                          (lambda: sqt.render_lens_rgb8(None, cam, 8, (W, H), subrays=4, motion=cam), "motion must be a Motion"),
                          (lambda: sqt.render_lens_rgb8(None, cam, 8, (W, H), subrays=4, motion=unchecked), "time_jitter"),
                          (lambda: next(sqt.render_adaptive(None, cam, 8, (W, H), 0.5, first=2, step=2, lens=ln, subrays=4, motion=3)), "motion must be a Motion")):
        with pytest.raises(E, match=message):
            call()
    with pytest.raises(ValueError, match="need a lens"):
        next(sqt.render_adaptive(None, cam, 8, (W, H), 0.5, motion=m))


def test_cli_shutter_flags(sqt, tmp_path):
    cli = importlib.import_module("squigly-trace_amd.cli")
    camera = os.path.join(ROOT, "data", "camera")
    text = open(camera, "rb").read()
    a = cli.parse_args(["--shutter-camera", camera])
    assert a.shutter_camera == text and a.shutter_jitter is None and a.subrays is None
    ln = cli.lens_of(a)
    assert (ln.jitter, ln.aperture, ln.focus) == (0.0, 0.0, 1.0)                # alone, --shutter-camera means Lens(jitter=0)
    a = cli.parse_args(["-s", "8", "--shutter-camera", camera, "--shutter-jitter", "0.5", "--aa", "0.5", "--subrays", "4", "--aperture", "0.1",
                        "--focus", "3", "--depth", "5", "--sky", "1,1,1"])
    ln = cli.lens_of(a)
    assert (a.shutter_jitter, a.subrays, ln.jitter, ln.focus, a.depth) == (0.5, 4, 0.5, 3.0, 5) and abs(ln.aperture - 0.1) < 1e-7
    assert cli.parse_args(["--shutter-camera", camera, "--shutter-jitter", "0"]).shutter_jitter == 0.0
    assert cli.lens_of(cli.parse_args([])) is None and cli.parse_args(["--aa"]).shutter_camera is None
    broken = tmp_path / "broken"
    broken.write_text("0 7 0.75\n1.57 0\n")
    for bad in (["--shutter-jitter", "0.5"], ["--aa", "--shutter-jitter", "0.5"], ["--shutter-camera", str(tmp_path / "none")],
                ["--shutter-camera", str(broken)], ["--shutter-camera", camera, "--shutter-jitter", "1.5"],
                ["--shutter-camera", camera, "--shutter-jitter", "-0.1"], ["--shutter-camera", camera, "--shutter-jitter", "nan"],
                ["--shutter-camera", camera, "--cast"], ["--shutter-camera", camera, "--views", camera],
                ["--shutter-camera", camera, "--adaptive", "0.5"], ["--shutter-camera", camera, "--preview-every", "2"],
                ["--shutter-camera", camera, "--focus", "3"], ["-s", "10", "--shutter-camera", camera, "--subrays", "4"],
                ["--shutter-camera", camera, "--subrays", "0"], ["--subrays", "4"]):
        with pytest.raises(SystemExit):
            cli.parse_args(bad)
