"""Anti-aliasing and depth of field without a GPU: the numpy restatement of include/squigly_lens.h pinned to the oracle where the two
meet, what its inputs cover, and the surface of libsquigly_lens.so -- the batch planner (also under the sanitizers, as a program
of its own), the header, the exports, the ids, every refusal that needs no device, the Python layer's refusals and the CLI's flags."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import lens_restatement as LR
import library_surface as LS
from render_options import THREADS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NO_DEVICE = 1 << 20         # a device number no machine has: a call the checks let through by mistake fails there, before any launch
W, H = LR.W, LR.H


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.fixture(scope="module")
def lens(sqt):
    mod = importlib.import_module("squigly-trace_amd.lens")
    mod.lib()
    return mod


@pytest.fixture(scope="module")
def room():
    return LR.room()


# ---- (a) no jitter, no aperture: makeRay's ray and the frame's seeds ----
@pytest.mark.parametrize("R", [1, 2, 4, 8])
def test_plain_lens_is_make_ray_and_the_frames_seeds(O, room, R):
    _, cam = room
    o, d, s = LR.rays(cam, LR.PLAIN, LR.S, R, W, H)
    want = [O.make_ray(W, H, y, x, cam) for y in range(W) for x in range(H)]
    wo, wd = np.array([r[0] for r in want], f32), np.array([r[1] for r in want], f32)
    for r in range(R):
        assert np.array_equal(bits(o[r]), bits(wo)) and np.array_equal(bits(d[r]), bits(wd))
    n = LR.S // R
    frame = np.array([LR.S * (x + y * W) for y in range(W) for x in range(H)], np.int64)
    assert np.array_equal(s, frame[None, :] + n * np.arange(R, dtype=np.int64)[:, None])
    # the union over r, each sub-ray taking n consecutive seeds, is the frame's own seeds, S * (x + y * w) + k (src/Lib.hs:85), pixel by pixel
    every = np.sort((s[:, :, None] + np.arange(n)[None, None, :]).transpose(1, 0, 2).reshape(W * H, LR.S), axis=1)
    assert np.array_equal(every, frame[:, None] + np.arange(LR.S)[None, :])


# ---- (b) R = 1: the oracle's frame ----
def test_one_plain_sub_ray_is_the_oracles_frame(room):
    c, cam = room
    tr = LR.trails(c.ob, c.flat, cam, LR.PLAIN, 3, 1, W, H)
    _, _, avg, rgb = LR.frame(tr, 3, 3)
    ref_avg, ref_rgb, _ = c.ob.render(cam, 3, W, H, threads=THREADS)
    assert np.array_equal(bits(avg.reshape(W, H, 3)), bits(ref_avg))
    assert np.array_equal(rgb.reshape(W, H, 3), ref_rgb)
    assert (ref_rgb.sum(-1) > 0).any()


# ---- (c) the thin lens: the sub-rays of a pixel meet on the plane in focus ----
def test_sub_rays_meet_on_the_focal_plane(O, room):
    """fp32 rounding over about ten operations is about 6e-7 relative; 1e-5 * max(1, |coordinate|) leaves a margin of 16 over that."""
    _, cam = room
    lens = LR.LENSES["dof"]
    a, focus = f32(lens[1]), f32(lens[2])
    pos, _ = O.camera_arrays(cam)
    worst = 0.0
    for y in range(W):
        for x in range(H):
            _, d0 = O.make_ray(W, H, y, x, cam)
            target = pos.astype(np.float64) + float(focus) * d0.astype(np.float64)
            for r in range(4):
                o, d, _, (xs, ys, lx, ly) = LR.sub_ray(cam, lens, LR.S, 4, W, H, y, x, r)
                at = o.astype(np.float64) + float(focus) * d.astype(np.float64)
                err = np.abs(at - target) / np.maximum(1.0, np.abs(target))
                worst = max(worst, float(err.max()))
                assert (err <= 1e-5).all(), (y, x, r, at, target)
                assert float(lx) ** 2 + float(ly) ** 2 <= float(a) ** 2 * (1 + 1e-6)
                assert xs == f32(x) and ys == f32(y)
    print(f"largest distance from the focal point, relative: {worst:.3g}")
    # the lens points differ between the sub-rays of a pixel and between pixels
    pts = {tuple(LR.sub_ray(cam, lens, LR.S, 4, W, H, 3, 5, r)[0]) for r in range(4)}
    assert len(pts) == 4


def test_jitter_stays_inside_the_pixel(room):
    _, cam = room
    seen = []
    for jitter in (1.0, 0.5):
        for y in (0, 7, W - 1):
            for x in range(H):
                for r in range(8):
                    _, _, _, (xs, ys, _, _) = LR.sub_ray(cam, (jitter, 0.0, 1.0), LR.S, 8, W, H, y, x, r)
                    assert f32(x) <= xs <= f32(x) + f32(jitter) and f32(y) <= ys <= f32(y) + f32(jitter)
                    seen.append((float(xs) - x, float(ys) - y))
    seen = np.array(seen)
    assert seen.min() < 0.02 and seen.max() > 0.98 and abs(seen[: len(seen) // 2].mean() - 0.5) < 0.03      # the draws fill the square


# ---- (d) the inputs bite ----
def coverage(room, lens, R):
    c, cam = room
    o, d, _ = LR.rays(cam, lens, LR.S, R, W, H)
    tri = LR.first_hits(c.ob, o, d)                       # [R, P]
    hit = tri >= 0
    mixed = int((hit.any(0) & ~hit.all(0)).sum())
    several = int(sum(1 for p in range(tri.shape[1]) if hit[:, p].all() and len(set(tri[:, p])) > 1))
    return mixed, several


def test_jittered_sub_rays_straddle_edges(room):
    """Counted on the CPU oracle when the feature was specified: 30 pixels whose four sub-rays mix hits and misses and 121 all-hit
    pixels whose sub-rays hit more than one triangle (R = 8: 38 and 131)."""
    mixed, several = coverage(room, LR.LENSES["aa"], 4)
    print(f"R = 4, jitter 1: {mixed} mixed pixels, {several} all-hit pixels with more than one triangle")
    assert mixed >= 20 and several >= 80


def test_lens_sub_rays_straddle_edges(room):
    """Counted likewise with no jitter, aperture 0.1 and focus 3: 104 all-hit pixels whose sub-rays hit more than one triangle."""
    _, several = coverage(room, LR.LENSES["dof"], 4)
    print(f"R = 4, aperture 0.1, focus 3: {several} all-hit pixels with more than one triangle")
    assert several >= 80


def test_fold_order_and_carry():
    """fold() is a left fold in sub-ray order that starts at s_0 (not at +0 + s_0), and ranges carry on bit for bit."""
    rng = np.random.default_rng(7)
    parts = (rng.standard_normal((8, 5, 3)) * 10.0 ** rng.integers(-3, 4, (8, 5, 3))).astype(f32)
    parts[0, 0] = -0.0
    s, q, avg = LR.fold(parts, 8)
    want = parts[0].copy()
    for r in range(1, 8):
        want = (want + parts[r]).astype(f32)
    assert np.array_equal(bits(s), bits(want))
    s1, q1, _ = LR.fold(parts, 8, (0, 3))
    s2, q2, avg2 = LR.fold(parts, 8, (3, 8), s1, q1)
    assert np.array_equal(bits(s2), bits(s)) and np.array_equal(bits(q2), bits(q)) and np.array_equal(bits(avg2), bits(avg))
    one = LR.fold(parts[:1], 8)
    assert np.array_equal(bits(one[0]), bits(parts[0])) and np.signbit(one[0][0]).all()       # s_0 itself: -0 stays -0
    rev, _, _ = LR.fold(parts[::-1], 8)
    assert not np.array_equal(bits(rev), bits(s))                                             # the order matters in fp32


# ---- (e) the library's surface ----
def header_text():
    return open(os.path.join(ROOT, "include", "squigly_lens.h")).read()


def test_header_functions_are_exported(lens):
    declared = LS.check_exports(lens, "squigly_lens.h", "sq_lens_")          # (and nothing of the other libraries' leaks out of this one)
    assert {"sq_lens_rays_device", "sq_lens_fold_device", "sq_lens_render_device", "sq_lens_plan", "sq_lens_work_bytes",
            "sq_lens_last_error", "sq_lens_build_id"} == declared


def test_header_carries_the_contract():
    text = header_text()
    for line in ("base   = S * (x + y * w) + r * n",
                 "m0..m3 = the first four outputs of mkTFGen (NOT base)",
                 "xs     = fromIntegral x + jitter * random01 m0",
                 "ys     = fromIntegral y + jitter * random01 m1",
                 "xoffs  = (xs - ww / 2) / ww ;  yoffs = (hh / 2 - ys) / hh",
                 "aperture == 0:  o = pos cam ;  dloc = V3 1 xoffs yoffs",
                 "rad = aperture * sqrt (random01 m2) ;  th = 2 * pi * random01 m3",
                 "lx = rad * cos th ;  ly = rad * sin th",
                 "o    = pos cam + (V3 0 lx ly `rotVert` rotation cam)",
                 "dloc = V3 1 (xoffs - lx / focus) (yoffs - ly / focus)",
                 "d = dloc `rotVert` rotation cam",
                 "sum  = s_0 ;  sum = sum + s_r  for r = 1 .. R-1 ;  sum2 likewise of s_r * s_r",
                 "avg  = (1 / (float) S) *^ sum ;  rgb = rgbFloatToPixelRGB avg"):
        assert line in text, line
    for word in ("INDEX WIDTHS", "2^31 - 1", "HOST WAIT", "44 bytes", "Out of scope"):
        assert word in text, word


def test_main_library_did_not_gain_the_lens(sqt, lens):
    for h in ("squigly_hip.h", "squigly_host.h", "squigly_denoise.h"):
        assert "sq_lens" not in open(os.path.join(ROOT, "include", h)).read(), h
    assert not [s for s in sqt.EXPORTED_SYMBOLS if "lens" in s]
    nm = subprocess.check_output(["nm", "-D", "--defined-only", sqt.LIB_PATH]).decode()
    assert "sq_lens" not in nm
    b = LS.build_module()
    mine = {"sq_lens.hip", "sq_lens_plan.h", "../../include/squigly_lens.h"}
    assert not mine & set(LS.files(b, "main", "denoise"))
    assert mine <= set(LS.files(b, "lens"))
    LS.check_client(lens.LIB_PATH, True)                                        # a client of the main library, found beside it


def test_ids_are_separate(lens, sqt, tmp_path):
    # the main library's and the denoiser's ids stay; the planner is text the two later lens libraries share, and their ids follow it
    LS.check_ids(LS.build_module(), "lens", lens, sqt, tmp_path,
                 [("sq_lens.hip", {"lens"}), ("sq_lens_plan.h", {"lens", "mlens", "shutter"})])


# ---- the planner ----
P0 = W * H                                  # 384 pixels: 16 896 bytes a sub-ray
PLAN_CASES = [
    # P, r_begin, r_end, work_bytes                                         what
    (P0, 0, 8, 8 * 16896),                                                # exact: one batch
    (P0, 0, 8, 3 * 16896),                                                # ragged: 3, 3, 2
    (P0, 0, 8, 16896),                                                    # one sub-ray at a time
    (P0, 0, 8, 2 * 16896 - 1),                                            # a byte short of two
    (P0, 3, 8, 3 * 16896),                                                # a range that starts above 0: 3, 2
    (P0, 0, 8, 1 << 40),                                                  # more room than the range needs
    (35, 0, 3, 2 * (288 + 3 * 432)),                                      # 35 pixels: the arrays are padded to 16 bytes
    (35, 0, 3, 44 * 35 * 3),                                              # 44 bytes a ray is not enough for three once padded
    (1, 0, 5, 64),                                                        # one pixel: 16 + 3 * 16 bytes a sub-ray
    (2 ** 31 - 1, 0, 4, 44 * (2 ** 31 - 1) + 64),                          # the largest P: one sub-ray a batch, whatever the room
    (2 ** 31 - 1, 0, 4, 1 << 50),
    (2 ** 30, 0, 4, 1 << 50),                                             # P * nb <= 2^31 - 1 caps the batch at one sub-ray
    (2 ** 30 - 1, 0, 4, 1 << 50),                                         # ... and here at two
    (1, 0, 2 ** 31 - 1, 64),                                              # 2^31 - 1 batches: counted, not listed
    (P0, 0, 8, 16895),                                                    # refused: too small
    (P0, 0, 8, 0),
    (0, 0, 8, 1 << 20), (-5, 0, 8, 1 << 20),                              # refused: P
    (2 ** 31, 0, 8, 1 << 50),                                             # refused: beyond the pixel index
    (P0, -1, 8, 1 << 20), (P0, 4, 4, 1 << 20), (P0, 5, 4, 1 << 20),        # refused: the range
]
PLAN_WANT = {0: [(0, 8)], 1: [(0, 3), (3, 6), (6, 8)], 2: [(r, r + 1) for r in range(8)], 3: [(r, r + 1) for r in range(8)],
             4: [(3, 6), (6, 8)], 5: [(0, 8)], 6: [(0, 2), (2, 3)], 7: [(0, 2), (2, 3)], 8: [(r, r + 1) for r in range(5)],
             9: [(r, r + 1) for r in range(4)], 10: [(r, r + 1) for r in range(4)], 11: [(r, r + 1) for r in range(4)],
             12: [(0, 2), (2, 4)]}
PLAN_REFUSED = {14: "too small", 15: "too small", 16: "at least 1", 17: "at least 1", 18: r"exceed 2\^31 - 1", 19: "bad sub-ray range",
                20: "bad sub-ray range", 21: "bad sub-ray range"}


def test_work_bytes(lens):
    wb = lens.work_bytes
    assert wb(P0, 1) == 44 * P0 == 16896 and wb(P0, 3) == 3 * 16896
    assert wb(35, 1) == 288 + 3 * 432 and wb(35, 1) >= 44 * 35 and wb(1, 1) == 64
    sizes = [1, 2, 3, 35, 63, 64, 65, 384, 1000, 2 ** 20]
    for p in sizes:
        for n0, n1 in zip(sizes, sizes[1:]):
            if p * n1 <= 2 ** 31 - 1:
                assert 44 * p * n0 <= wb(p, n0) <= wb(p, n1) and wb(n0, p) <= wb(n1, p) and wb(p, n0) < 44 * p * n0 + 64
    assert wb(0, 1) == wb(1, 0) == wb(-1, 1) == wb(1, -1) == 0
    assert wb(2 ** 31 - 1, 1) > 0 and wb(2 ** 31, 1) == 0 and wb(2 ** 30, 2) == 0 and wb(2 ** 30, 1) > 0 and wb(2 ** 16, 2 ** 15) == 0
    assert wb(2 ** 16, 2 ** 15 - 1) > 0


def test_plan(lens):
    assert sorted(list(PLAN_WANT) + list(PLAN_REFUSED) + [13]) == list(range(len(PLAN_CASES)))
    for i, (p, r0, r1, nbytes) in enumerate(PLAN_CASES):
        if i in PLAN_REFUSED:
            with pytest.raises(lens.N.SquiglyError, match=PLAN_REFUSED[i]):
                lens.plan(p, r0, r1, nbytes)
            continue
        if i == 13:
            assert lens.lib().sq_lens_plan(p, r0, r1, nbytes, None, 0) == 2 ** 31 - 1
            continue
        got = lens.plan(p, r0, r1, nbytes)
        assert got == PLAN_WANT[i], (i, got)
        # the batches tile the range in order, each fits the workspace, and one more sub-ray in the first would not
        assert got[0][0] == r0 and got[-1][1] == r1 and all(a[1] == b[0] for a, b in zip(got, got[1:]))
        nb = got[0][1] - got[0][0]
        assert all(0 < lens.work_bytes(p, b - a) <= nbytes and b - a <= nb for a, b in got)
        if nb < r1 - r0:
            assert lens.work_bytes(p, nb + 1) == 0 or lens.work_bytes(p, nb + 1) > nbytes
    # cap: a short array gets the first batches, and the count is the whole plan's
    out = (C.c_int32 * 5)(*([-7] * 5))
    assert lens.lib().sq_lens_plan(P0, 0, 8, 3 * 16896, out, 2) == 3 and list(out) == [0, 3, 3, 6, -7]


def test_planner_under_address_and_undefined_behaviour_sanitizers(lens, tmp_path):
    """tests/lens_plan_main.cpp (its own main over csrc/sq_lens_plan.h, the planner's host code) compiled with
    -fsanitize=address,undefined and run as a child process, once, over PLAN_CASES: exit 0, nothing on stderr, and line by line
    what the library plans."""
    exe = str(tmp_path / "lens_plan_main")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-static-libasan", "-static-libubsan",      # the runtimes inside the program: nothing to order at load time
                           os.path.join(ROOT, "tests", "lens_plan_main.cpp"), "-o", exe])
    args = [str(v) for case in PLAN_CASES for v in case]
    r = subprocess.run([exe] + args, capture_output=True)
    assert r.returncode == 0 and r.stderr == b"", (r.returncode, r.stderr[-2000:])
    lines = r.stdout.decode().splitlines()
    assert len(lines) == len(PLAN_CASES)
    for i, line in enumerate(lines):
        if i in PLAN_REFUSED:
            assert line.startswith("refused: ") and re.search(PLAN_REFUSED[i], line), (i, line)
        elif i == 13:
            assert line.startswith(f"plan {2 ** 31 - 1}: 0-1 1-2 ") and line.endswith(" 63-64"), line
        else:
            assert line == f"plan {len(PLAN_WANT[i])}: " + " ".join(f"{a}-{b}" for a, b in PLAN_WANT[i]), (i, line)


# ---- refusals: nothing here reaches a device, the buffer pointers are numbers that are never followed ----
BUF = {name: 0x10000000 + i * 0x1000000 for i, name in enumerate(("org", "dir", "seed", "part", "sum", "sum2", "avg", "rgb", "work"))}
SCENE = 0x7000000           # stands for a scene: the checks never follow it either
FAR = {name: (i + 1) << 40 for i, name in enumerate(BUF)}          # far enough apart for the largest calls the index widths allow


def frame_call(sqt, lens, which, cam=True, lens_values=(1.0, 0.0, 1.0), null_lens=False, S=8, R=4, r=(0, 4), w=W, h=H,
               shard=None, work_bytes=None, device=NO_DEVICE, **ptr):
    L = lens.lib()
    a = {**BUF, **ptr}
    c = sqt.load_camera(os.path.join(ROOT, "data", "camera"))
    ln = lens.Lens.__new__(lens.Lens)                       # unchecked values: the library's own checks are what is under test
    C.Structure.__init__(ln, *lens_values)
    sh = sqt.Shard(*(shard or (w if w > 0 else 1, 0, 1)))
    head = [C.byref(c) if cam else None, None if null_lens else C.byref(ln), S, R, r[0], r[1], w, h, sh]
    if which == "rays":
        rc = L.sq_lens_rays_device(device, *head, a["org"], a["dir"], a["seed"], None)
    else:
        wb = lens.work_bytes(W * H, 1) if work_bytes is None else work_bytes
        rc = L.sq_lens_render_device(a.get("scene", SCENE), *head, a["work"], wb, a["sum"], a["sum2"], a["avg"], a["rgb"], None)
    return rc, L.sq_lens_last_error().decode()


nan, inf = float("nan"), float("inf")
FRAME_REFUSALS = [
    (dict(cam=False), "null argument"), (dict(null_lens=True), "null argument"),
    (dict(S=0), "at least 1"), (dict(R=0), "at least 1"), (dict(S=-8), "at least 1"), (dict(S=8, R=3), "must divide"),
    (dict(S=4, R=8, r=(0, 8)), "must divide"),
    (dict(r=(-1, 4)), "bad sub-ray range"), (dict(r=(2, 2)), "bad sub-ray range"), (dict(r=(3, 2)), "bad sub-ray range"),
    (dict(r=(0, 5)), "bad sub-ray range"),
    (dict(lens_values=(-0.1, 0.0, 1.0)), "jitter"), (dict(lens_values=(1.5, 0.0, 1.0)), "jitter"), (dict(lens_values=(nan, 0.0, 1.0)), "jitter"),
    (dict(lens_values=(inf, 0.0, 1.0)), "jitter"),
    (dict(lens_values=(1.0, -0.5, 1.0)), "aperture"), (dict(lens_values=(1.0, nan, 1.0)), "aperture"), (dict(lens_values=(1.0, inf, 1.0)), "aperture"),
    (dict(lens_values=(1.0, 0.1, 0.0)), "focus"), (dict(lens_values=(1.0, 0.1, -3.0)), "focus"), (dict(lens_values=(1.0, 0.1, nan)), "focus"),
    (dict(lens_values=(1.0, 0.1, inf)), "focus"),
    (dict(w=0), "at least 1"), (dict(h=0), "at least 1"), (dict(h=-2), "at least 1"),
    (dict(shard=(2, 3, 3)), "bad shard"), (dict(shard=(0, 0, 1)), "bad shard"),
    (dict(w=46341, h=46341, work_bytes=1 << 50), r"exceed 2\^31 - 1 pixels"),
]
RAYS_REFUSALS = FRAME_REFUSALS + [
    (dict(org=None), "null argument"), (dict(dir=None), "null argument"), (dict(seed=None), "null argument"),
    (dict(w=1024, h=1024, S=4096, R=4096, r=(0, 2048)), r"exceed 2\^31 - 1 ray slots"),         # 2^20 pixels x 2^11 sub-rays
    (dict(w=1024, h=1024, S=4096, R=4096, r=(2048, 4096)), r"exceed 2\^31 - 1 ray slots"),
    (dict(dir=BUF["org"] + 12 * W * H * 4 - 4), "d_org and d_dir overlap"), (dict(seed=BUF["org"]), "d_org and d_seed overlap"),
    (dict(seed=BUF["dir"] - 8), "d_dir and d_seed overlap"),
]
RENDER_REFUSALS = FRAME_REFUSALS + [
    (dict(scene=None), "null argument"), (dict(work=None), "null argument"), (dict(sum=None), "null argument"),
    (dict(work_bytes=16895), "too small"), (dict(work_bytes=0), "too small"),
    (dict(work=BUF["work"] + 8), "16-byte aligned"),
    (dict(sum2=BUF["sum"] + 12), "d_sum and d_sum2 overlap"), (dict(avg=BUF["sum"]), "d_sum and d_avg overlap"),
    (dict(rgb=BUF["avg"] + 12 * W * H - 1), "d_avg and d_rgb overlap"), (dict(rgb=BUF["sum2"]), "d_sum2 and d_rgb overlap"),
    (dict(work=BUF["sum"] - 16), "d_sum and d_work overlap"), (dict(avg=BUF["work"] + 16896 - 16), "d_avg and d_work overlap"),
]


@pytest.mark.parametrize("kw, message", RAYS_REFUSALS, ids=[f"{i:02d}-{m[:12]}" for i, (_, m) in enumerate(RAYS_REFUSALS)])
def test_rays_refusals_need_no_gpu(sqt, lens, kw, message):
    rc, err = frame_call(sqt, lens, "rays", **kw)
    assert rc != 0 and re.search(message, err), err


@pytest.mark.parametrize("kw, message", RENDER_REFUSALS, ids=[f"{i:02d}-{m[:12]}" for i, (_, m) in enumerate(RENDER_REFUSALS)])
def test_render_refusals_need_no_gpu(sqt, lens, kw, message):
    rc, err = frame_call(sqt, lens, "render", **kw)
    assert rc != 0 and re.search(message, err), err


def test_what_is_allowed_gets_past_the_checks(sqt, lens):
    """The largest batch, the open aperture, jitter 0 and 1, no optional buffer: on a device that does not exist they fail at the
    first runtime call, and with its message.  An empty shard is no error and touches nothing."""
    for kw in (dict(), dict(lens_values=(0.0, 0.0, -1.0)), dict(lens_values=(1.0, 0.25, 3.0)), dict(lens_values=(-0.0, 0.0, nan)),
               dict(w=1024, h=1024, S=4096, R=4096, r=(0, 2047), **FAR), dict(w=46340, h=46340, S=1, R=1, r=(0, 1), **FAR), dict(r=(3, 4))):
        rc, err = frame_call(sqt, lens, "rays", **kw)
        assert rc != 0 and "hipSetDevice" in err, err
    for kw in (dict(), dict(sum2=None, avg=None, rgb=None), dict(work_bytes=1 << 20), dict(r=(1, 3))):
        rc, err = frame_call(sqt, lens, "render", **kw)
        assert rc != 0 and "hipPointerGetAttributes" in err, err
    for which in ("rays", "render"):
        assert frame_call(sqt, lens, which, w=4, shard=(2, 2, 3))[0] == 0


def test_fold_refusals(lens):
    L = lens.lib()
    B = BUF
    ok = dict(P=384, S=8, r=(0, 4), part=B["part"], sum=B["sum"], sum2=B["sum2"], avg=B["avg"], rgb=B["rgb"])
    cases = [(dict(part=None), "null argument"), (dict(sum=None), "null argument"), (dict(P=0), "at least 1"), (dict(P=-4), "at least 1"),
             (dict(S=0), "at least 1"), (dict(r=(-1, 4)), "bad sub-ray range"), (dict(r=(4, 4)), "bad sub-ray range"),
             (dict(r=(0, 9)), "bad sub-ray range"), (dict(P=2 ** 31), r"exceed 2\^31 - 1 pixels"),
             (dict(P=2 ** 20, S=4096, r=(0, 2048)), r"exceed 2\^31 - 1 ray slots"),
             (dict(sum=B["part"] + 12 * 384 * 4 - 4), "d_part and d_sum overlap"), (dict(sum2=B["sum"]), "d_sum and d_sum2 overlap"),
             (dict(avg=B["sum2"] + 12), "d_sum2 and d_avg overlap"), (dict(rgb=B["part"]), "d_part and d_rgb overlap")]
    for kw, message in cases:
        a = {**ok, **kw}
        rc = L.sq_lens_fold_device(NO_DEVICE, a["P"], a["S"], a["r"][0], a["r"][1], a["part"], a["sum"], a["sum2"], a["avg"], a["rgb"], None)
        assert rc != 0 and re.search(message, L.sq_lens_last_error().decode()), (kw, L.sq_lens_last_error())
    far = {k: FAR[k] for k in ("part", "sum", "sum2", "avg", "rgb")}
    for kw in (dict(), dict(sum2=None, avg=None, rgb=None), dict(r=(3, 8)), dict(P=2 ** 31 - 1, r=(0, 1), **far), dict(P=2 ** 20, S=4096, r=(0, 2047), **far)):
        a = {**ok, **kw}
        rc = L.sq_lens_fold_device(NO_DEVICE, a["P"], a["S"], a["r"][0], a["r"][1], a["part"], a["sum"], a["sum2"], a["avg"], a["rgb"], None)
        assert rc != 0 and "hipSetDevice" in L.sq_lens_last_error().decode()


# ---- the Python layer ----
def test_python_refusals(sqt, lens):
    E = sqt.SquiglyError
    assert (sqt.Lens().jitter, sqt.Lens().aperture, sqt.Lens().focus) == (1.0, 0.0, 1.0)
    ln = sqt.Lens(jitter=0.5, aperture=0.25, focus=3)
    assert (ln.jitter, ln.aperture, ln.focus) == (0.5, 0.25, 3.0) and "0.25" in repr(ln)
    sqt.Lens(0, 0, -1)                                                     # the focus is read only when the aperture is open
    for kw, message in ((dict(jitter=-0.1), "jitter"), (dict(jitter=1.01), "jitter"), (dict(jitter=nan), "jitter"), (dict(jitter="1"), "jitter must be a number"),
                        (dict(jitter=True), "jitter must be a number"), (dict(aperture=-1), "aperture"), (dict(aperture=inf), "aperture"),
                        (dict(aperture=nan), "aperture"), (dict(aperture=None), "aperture must be a number"),
                        (dict(aperture=0.1, focus=0), "focus"), (dict(aperture=0.1, focus=inf), "focus"), (dict(aperture=0.1, focus=nan), "focus")):
        with pytest.raises(E, match=message):
            sqt.Lens(**kw)
    fa = lens.frame_args
    assert fa(ln, 8, 4) == (8, 4, 0, 4) and fa(ln, 8, 4, (1, 3)) == (8, 4, 1, 3) and fa(ln, np.int32(6), 3, [2, 3]) == (6, 3, 2, 3)
    for args, message in (((None, 8, 4), "lens must be a Lens"), (((1.0, 0.0, 1.0), 8, 4), "lens must be a Lens"), ((ln, 0, 1), "at least 1"),
                          ((ln, 8, 0), "at least 1"), ((ln, 8.0, 4), "samples must be an integer"), ((ln, 8, True), "subrays must be an integer"),
                          ((ln, 8, 3), "must divide"), ((ln, 8, 4, (0, 5)), "bad sub-ray range"), ((ln, 8, 4, (2, 2)), "bad sub-ray range"),
                          ((ln, 8, 4, (-1, 2)), "bad sub-ray range"), ((ln, 8, 4, 3), "r_range must be"), ((ln, 8, 4, (0, 1.5)), "must be an integer")):
        with pytest.raises(E, match=message):
            fa(*args)
    # a scene that was never uploaded: whatever gets past its refusal would fail in some other way
    ds = object.__new__(sqt.DeviceScene)
    ds.device, ds._h = 0, None
    cam = sqt.load_camera(os.path.join(ROOT, "data", "camera"))
    for call, message in ((lambda: ds.render_lens(cam, ln, 8, 3, W, H), "must divide"),
                          (lambda: ds.render_lens(cam, None, 8, 4, W, H), "lens must be a Lens"),
                          (lambda: ds.render_lens(cam, ln, 8, 4, W, H, work_mb=0), "work_mb"),
                          (lambda: ds.render_lens(cam, ln, 8, 4, W, H, work_mb=nan), "work_mb"),
                          (lambda: ds.render_lens(cam, ln, 8, 4, W, H, shard=(2, 3, 3)), "bad shard"),
                          (lambda: ds.render_lens(cam, ln, 8, 4, W, H, r_range=(2, 4)), "needs the sums"),
                          (lambda: ds.render_lens(cam, ln, 4, 4, 46341, 46341), r"exceed 2\^31 - 1 pixels"),
                          (lambda: ds.lens_rays(cam, ln, 8, 4, W, H, r_range=(0, 9)), "bad sub-ray range"),
                          (lambda: ds.lens_rays(cam, ln, 8, 4, W, H, shard=(0, 0, 1)), "bad shard"),
                          (lambda: ds.lens_rays(cam, ln, 4096, 4096, 1024, 1024, r_range=(0, 2048)), r"exceed 2\^31 - 1 ray slots"),
                          (lambda: sqt.render_lens_rgb8(None, cam, 8, (W, H), subrays=3), "must divide"),
                          (lambda: sqt.render_lens_rgb8(None, cam, 8, (W, H), lens=(1, 0, 1)), "lens must be a Lens"),
                          (lambda: sqt.render_lens_rgb8(None, cam, 8, (W, H), depth=9), "depth")):
        with pytest.raises(E, match=message):
            call()


def test_cli_lens_flags(sqt):
    cli = importlib.import_module("squigly-trace_amd.cli")
    a = cli.parse_args(["--aa"])
    assert a.aa == 1.0 and a.subrays is None and a.aperture is None and a.focus is None
    ln = cli.lens_of(a)
    assert (ln.jitter, ln.aperture, ln.focus) == (1.0, 0.0, 1.0)
    a = cli.parse_args(["-s", "8", "--aa", "0.5", "--subrays", "4", "--aperture", "0.1", "--focus", "3"])
    ln = cli.lens_of(a)
    assert (a.subrays, ln.jitter, ln.focus) == (4, 0.5, 3.0) and abs(ln.aperture - 0.1) < 1e-7
    ln = cli.lens_of(cli.parse_args(["--aperture", "0.2"]))
    assert (ln.jitter, ln.focus) == (0.0, 1.0) and abs(ln.aperture - 0.2) < 1e-7
    assert cli.lens_of(cli.parse_args([])) is None
    assert cli.parse_args(["--aa", "--depth", "5", "--sky", "1,1,1"]).depth == 5           # depth and sky apply to a lens frame
    views = os.path.join(ROOT, "data", "camera")
    for bad in (["--aa", "1.5"], ["--aa", "-0.5"], ["--aa", "x"], ["--subrays", "4"], ["--focus", "3"], ["--aa", "--focus", "3"],
                ["--aa", "--subrays", "0"], ["-s", "10", "--aa", "--subrays", "4"], ["--aperture", "-1"], ["--aperture", "inf"],
                ["--aperture", "0.1", "--focus", "0"], ["--aperture", "0.1", "--focus", "inf"],
                ["--aa", "--cast"], ["--aperture", "0.1", "--cast"], ["--aa", "--views", views], ["--aa", "--adaptive", "0.5"],
                ["--aa", "--preview-every", "2"], ["--aperture", "0.1", "--adaptive", "0.5"]):
        with pytest.raises(SystemExit):
            cli.parse_args(bad)
