"""sq_temporal_accumulate_moving_device on the GPU: colour, variance, length, flags and the unpacked next block bit for bit (NaN = NaN)
against the numpy restatement (tests/moving_restatement.py), at the sizes where the window and the tile can go wrong, with both kernel
forms, with object and transform tables that sit between poison, and the driver on top (sqt.Temporal.step with a scene,
render_moving_sequence, the CLI) on the moving room (tests/moving_room.py)."""
import collections
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import moving_restatement as M
import moving_room as MR
import temporal_restatement as R
from bitcmp import same, same_exact
from conftest import DATA

pytestmark = pytest.mark.gpu
f32 = np.float32
G = collections.namedtuple("G", ["tri", "normal", "point"])
# 1 x 1, two pixels either way; a window (r = 3) larger than the image; one row wider than two waves; a tile crossed in both
# directions, so that halos cross image borders and tile borders; the room's size
SIZES = [(1, 1), (1, 2), (2, 1), (5, 7), (1, 130), (17, 67), (48, 64)]
SIZE_IDS = [f"{r}x{c}" for r, c in SIZES]
CAM = ((0, 0, 0), R.IDENTITY)
SIGMA_P = 0.05
INF = float("inf")
CLAMPS = [None, (1, 0.0), (2, 1.0), (3, INF), (3, 1.0), (1, INF), (2, 0.0)]           # (radius, k): every radius with k 0, 1 and +inf
FORMS = ("direct", "tiled")
GUARD = 64                                                                           # words of poison before and behind a table
INT_POISONS, FLOAT_POISONS = (0, 3, 2 ** 31 - 1), (float("nan"), 1.0e30, 0.0)


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def tp(sqt, torch):
    mod = importlib.import_module("squigly-trace_amd.temporal")
    mod.lib()
    return mod


def guarded_table(torch, values, fill):
    """A device copy of the 1-D array `values` that sits GUARD + 1 words into a larger allocation filled with `fill` (so it is not
    16-byte aligned either) and ends GUARD words before its end: what a read through a wrong index would find."""
    t = torch.from_numpy(np.ascontiguousarray(values)).cuda()
    whole = torch.full((GUARD + 1 + t.numel() + GUARD,), fill, dtype=t.dtype, device="cuda")
    view = whole[GUARD + 1:GUARD + 1 + t.numel()]
    view.copy_(t.reshape(-1))
    return view.view(*t.shape), whole


def dev(torch, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def gpu_frame(torch, fr):
    color, var, tri, nrm, pnt = (dev(torch, a) for a in fr)
    return color, var, G(tri, nrm, pnt)


def cam_of(sqt, cam):
    pos, rot = R.camera(cam)
    c = sqt.Camera()
    c.pos[:], c.rot[:] = [float(v) for v in pos], [float(v) for v in rot]
    return c


def prev_camera(rows, cols):
    """A previous camera under which most pixels find their history: a generic small move, or for a one-row or one-column image a
    step of a fraction of a pixel along the axis it has."""
    px, py = 4.0 / rows, 4.0 / cols
    if rows > 1 and cols > 1:
        return ((0.3, 0.37 * px, -0.21 * py), R.turned(0.01))
    return ((0, 0.3 * px, 0), R.IDENTITY) if cols > 1 else ((0, 0, -0.3 * py), R.IDENTITY) if rows > 1 else CAM


N_TRIS = 21                                             # the table's last entry is triangle 20's: n_tris - 1


def frames_for(rows, cols, seed):
    """(cur, prev, prev camera): the synthetic two-plane frames; in the current one a few pixels carry the triangle ids at the
    table's edge (n_tris - 1 is the strip's own; n_tris and INT32_MAX are beyond it), and -- from 17 x 67 up -- a hit pixel in the
    middle stands alone among misses: a window with no valid tap but its centre.  (At 1 x 1 the only pixel is such a window too.)"""
    pcam = prev_camera(rows, cols)
    bg = 0.0 if rows * cols <= 2 else 0.08
    cur, prev = R.synthetic(rows, cols, seed, CAM, 0.01, background=bg), R.synthetic(rows, cols, seed + 1, pcam, 0.01, background=bg)
    tri = M.scatter_triangles(cur[2], N_TRIS, seed + 2)
    lone = None
    if rows >= 9 and cols >= 9:                         # (at 5 x 7 the window is the whole image: that is its own case)
        lone = (rows // 2, cols // 2)
        mine = tri[lone]
        tri[lone[0] - 3:lone[0] + 4, lone[1] - 3:lone[1] + 4] = -1
        tri[lone] = mine if mine >= 0 else R.FAR_TRI
    hits = [tuple(p) for p in np.argwhere(tri >= 0) if tuple(p) != lone]
    if len(hits) >= 8:
        for (y, x), t in zip((hits[1], hits[len(hits) // 2], hits[-2]), (N_TRIS, 2 ** 31 - 1, N_TRIS - 1)):
            tri[y, x] = t
    return cur, prev, pcam


def call(tp, torch, sqt, cur, pcam, pblk, alpha=None, tables=None, clamp=None, form="auto", alias_var=False, **params):
    """One moving call through the Python layer; returns (out, out_var, out_len, flags) and the block it wrote."""
    color, var, g = gpu_frame(torch, cur)
    nxt = tp.history(*cur[2].shape, 0)
    kw = {}
    if tables is not None:
        kw.update(objects=tables[0], back=tables[1])
    if clamp is not None:
        kw.update(clamp=(clamp[1], clamp[0]), form=form)                # the Python layer's pair is (k, radius)
    if alias_var:
        kw.update(out=(torch.empty_like(color), var))
    got = tp.accumulate(color, var, g, None if pblk is None else cam_of(sqt, pcam), pblk, nxt, alpha=dev(torch, alpha), want_flags=True,
                        **kw, **params)
    if alias_var:
        assert got[1].data_ptr() == var.data_ptr()
    return got, nxt


def assert_result(torch, tp, got, blk, want, label):
    torch.cuda.synchronize()
    rows, cols = want["len"].shape
    for name, g, w in (("colour", got[0], want["color"]), ("variance", got[1], want["var"])):
        g = g.cpu().numpy()
        bad = ~((g.view(np.uint32) == w.view(np.uint32)) | (np.isnan(g) & np.isnan(w)))
        assert same(g, w), (label, name, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    assert np.array_equal(got[2].cpu().numpy(), want["len"]), (label, "length")
    gf = got[3].cpu().numpy()
    assert np.array_equal(gf, want["flags"]), (label, "flags", np.argwhere(gf != want["flags"])[:4].tolist())
    h = tp.unpack(blk, rows, cols)
    torch.cuda.synchronize()
    for name in R.BLOCK_FIELDS:
        g, w = getattr(h, name).cpu().numpy(), want["block"][name]
        assert (same(g, w) if w.dtype == f32 else np.array_equal(g, w)), (label, "block", name)


def first_block(torch, tp, fr):
    color, var, g = gpu_frame(torch, fr)
    blk = tp.history(*fr[2].shape, 0)
    tp.accumulate(color, var, g, None, None, blk, sigma_p=SIGMA_P)
    return blk


@pytest.mark.parametrize("rows, cols", SIZES, ids=SIZE_IDS)
def test_every_clamp_and_form_with_guarded_tables(sqt, torch, tp, rows, cols):
    """Every clamp in both kernel forms, with d_alpha, objects of every kind (-1, 0, n_objects - 1, n_objects, large positive and
    negative) and transform rows of every kind (identity, a rotation plus translation, NaN, infinite).  The tables sit between
    poison that changes from one clamp to the next: the result is the restatement's, which never sees it."""
    cur, prev, pcam = frames_for(rows, cols, 100 + rows)
    objects, back = M.tables(N_TRIS, 0)
    assert {-1, 0, 4, 5, 2 ** 31 - 1, -2 ** 31} <= set(objects.tolist()) and len(back) == 5      # n_objects - 1 = 4, n_objects = 5
    alpha = np.random.default_rng(rows * 1000 + cols).random((rows, cols)).astype(f32)
    pblk, pwant = first_block(torch, tp, prev), R.first_block(*prev)
    seen = 0
    for i, clamp in enumerate(CLAMPS):
        want = M.accumulate(*cur, pcam, pwant, alpha=alpha, objects=objects, back=back, clamp=clamp, sigma_p=SIGMA_P)
        seen |= int(np.bitwise_or.reduce(want["flags"].reshape(-1)))
        for form in FORMS if clamp is not None else ("auto",):
            ot, o_whole = guarded_table(torch, objects, INT_POISONS[i % 3])
            bt, b_whole = guarded_table(torch, back, FLOAT_POISONS[i % 3])
            got, nxt = call(tp, torch, sqt, cur, pcam, pblk, alpha=alpha, tables=(ot, bt), clamp=clamp, form=form, sigma_p=SIGMA_P)
            assert_result(torch, tp, got, nxt, want, (rows, cols, clamp, form))
            assert o_whole[:GUARD + 1].eq(INT_POISONS[i % 3]).all() and o_whole[-GUARD:].eq(INT_POISONS[i % 3]).all()
    if rows * cols >= 35:
        assert seen == M.BLENDED | M.CLAMPED | M.MOVED, seen
        tri = cur[2]
        y, x = rows // 2, cols // 2
        if rows >= 9 and cols >= 9:                                   # the hit pixel that stands alone
            assert tri[y, x] >= 0 and (tri[max(0, y - 3):y + 4, max(0, x - 3):x + 4] >= 0).sum() == 1
        assert (tri == N_TRIS).any() and (tri == 2 ** 31 - 1).any() and (tri == N_TRIS - 1).any()


@pytest.mark.parametrize("rows, cols", [(1, 1), (5, 7), (17, 67)], ids=["1x1", "5x7", "17x67"])
def test_no_history_and_the_lone_window(sqt, torch, tp, rows, cols):
    """prev = NULL under tables, a clamp and flags: the inputs come back and every flag is 0.  Then, with history and no misses
    around it, the lone pixel's window (n = 1, sd = 0: lo = hi = its own colour) clamps its history to the frame's colour."""
    cur, prev, pcam = frames_for(rows, cols, 200 + rows)
    objects, back = M.tables(N_TRIS, 8)
    got, nxt = call(tp, torch, sqt, cur, None, None, tables=(dev(torch, objects), dev(torch, back)), clamp=(3, 1.0), sigma_p=SIGMA_P)
    want = M.accumulate(*cur, None, None, objects=objects, back=back, clamp=(3, 1.0), sigma_p=SIGMA_P)
    assert not want["flags"].any() and same(want["color"], cur[0])
    assert_result(torch, tp, got, nxt, want, (rows, cols, "first frame"))
    if rows >= 9:
        y, x = rows // 2, cols // 2
        cur[0][y, x] = (0.5, 0.25, 2.0)                               # finite, so that the clamp compares
        pblk = first_block(torch, tp, prev)
        for form in FORMS:
            got, nxt = call(tp, torch, sqt, cur, CAM, pblk, clamp=(3, 1.0), form=form, sigma_p=SIGMA_P)
            want = M.accumulate(*cur, CAM, R.first_block(*prev), clamp=(3, 1.0), sigma_p=SIGMA_P)
            assert_result(torch, tp, got, nxt, want, (rows, cols, "lone", form))
        if want["flags"][y, x] & M.BLENDED:
            assert same(want["color"][y, x], cur[0][y, x])


def moving_cameras(rows, cols, n):
    px, py = 4.0 / rows, 4.0 / cols
    return [((0.02 * i, 0.45 * px * i, -0.3 * py * i), R.turned(0.004 * i)) for i in range(n)]


@pytest.mark.parametrize("rows, cols", [(17, 67), (48, 64)], ids=["17x67", "48x64"])
def test_chain_of_five_frames_under_a_back_per_frame(sqt, torch, tp, rows, cols):
    """Five frames through two blocks that take turns, the far wall (object 1) going through another small rigid move every frame,
    under a clamp and d_alpha, the variance written in place: every frame equals the restatement's chain."""
    cams = moving_cameras(rows, cols, 5)
    frames = [R.synthetic(rows, cols, 300 + i, cams[i], 0.01) for i in range(5)]
    alphas = [np.random.default_rng(310 + i).random((rows, cols)).astype(f32) * f32(0.5) for i in range(5)]
    objects, _ = M.tables(N_TRIS, 9)
    backs = [np.stack([M.IDENTITY_ROW, M.rigid(0.002 * i, (0.1, 1, 0.2), (0.0005 * i, 0.01 * i, -0.004)).reshape(12).astype(f32)])
             for i in range(5)]
    objects = np.where(objects > 1, -1, objects).astype(np.int32)
    params = dict(sigma_p=SIGMA_P, max_history=3, alpha_min=0.05)
    want = M.chain(frames, cams, alphas, objects=objects, backs=backs, clamp=(2, 1.5), **params)
    blocks = [tp.history(rows, cols, 0), tp.history(rows, cols, 0)]
    prev, prev_cam, ot = None, None, dev(torch, objects)
    for i, fr in enumerate(frames):
        color, var, g = gpu_frame(torch, fr)
        nxt = blocks[i & 1]
        got = tp.accumulate(color, var, g, prev_cam, prev, nxt, alpha=dev(torch, alphas[i]), objects=ot, back=backs[i], clamp=(1.5, 2),
                            want_flags=True, out=(torch.empty_like(color), var), form=FORMS[i & 1], **params)
        assert got[1].data_ptr() == var.data_ptr()
        assert_result(torch, tp, got, nxt, want[i], (rows, cols, "frame", i))
        prev, prev_cam = nxt, cam_of(sqt, cams[i])
    last = want[-1]["flags"]
    assert want[-1]["len"].max() == 3 and (last & M.MOVED).any() and (last & M.CLAMPED).any()


def test_more_tiles_than_blocks(sqt, torch, tp):
    """4100 x 65: 2 x 1025 tiles (the second column of tiles one pixel wide) against the 2048 blocks of a launch, so the tile loop
    runs more than once -- with the tiled form the staging buffer is then reused behind a barrier, which the small shapes never do.
    The wall goes through the identity and keeps its history down to the last rows."""
    rows, cols = 4100, 65
    pcam = ((0, 0.37 * 4.0 / rows, -0.21 * 4.0 / cols), R.IDENTITY)
    cur, prev = R.synthetic(rows, cols, 8, CAM, 0.01), R.synthetic(rows, cols, 9, pcam, 0.01)
    objects, back = M.tables(N_TRIS, 10)
    objects[R.FAR_TRI], objects[R.NEAR_TRI] = 0, 4
    pblk = first_block(torch, tp, prev)
    want = M.accumulate(*cur, pcam, R.first_block(*prev), objects=objects, back=back, clamp=(1, 1.0), sigma_p=SIGMA_P)
    assert (want["len"][-4:] == 2).any() and (want["len"][:4] == 2).any() and (want["flags"][-4:] & M.CLAMPED).any()
    for form in FORMS:
        got, nxt = call(tp, torch, sqt, cur, pcam, pblk, tables=(dev(torch, objects), dev(torch, back)), clamp=(1, 1.0), form=form,
                        sigma_p=SIGMA_P)
        assert_result(torch, tp, got, nxt, want, (rows, cols, form))


@pytest.mark.parametrize("rows, cols", [(5, 7), (17, 67), (48, 64)], ids=["5x7", "17x67", "48x64"])
def test_the_anchor(sqt, torch, tp, rows, cols):
    """With d_object, d_back, clamp and d_out_flags all NULL the new entry point writes the bytes of
    sq_temporal_accumulate_device: out, out_var, out_len and the whole next block, with and without history and d_alpha.  So it
    does with d_out_flags alone given -- the moving kernel without a clamp, where the other two calls run the static one -- and the
    flags are then the restatement's."""
    cur, prev, pcam = frames_for(rows, cols, 400 + rows)
    color, var, g = gpu_frame(torch, cur)
    alpha_host = np.random.default_rng(rows).random((rows, cols)).astype(f32)
    alpha = dev(torch, alpha_host)
    pblk, pwant = first_block(torch, tp, prev), R.first_block(*prev)
    par, cam, L = tp.make_params(sigma_p=SIGMA_P), cam_of(sqt, pcam), tp.lib()
    for prev_blk in (None, pblk):
        for al in (None, alpha):
            res = []
            for how in ("old", "new", "flags"):
                nxt = torch.full((tp.history_bytes(rows, cols),), 0xA5, dtype=torch.uint8, device="cuda")
                out = torch.empty((rows, cols, 3), dtype=torch.float32, device="cuda")
                out_v = torch.empty((rows, cols), dtype=torch.float32, device="cuda")
                out_l = torch.empty((rows, cols), dtype=torch.int32, device="cuda")
                flags = torch.full((rows, cols), 0xA5, dtype=torch.uint8, device="cuda") if how == "flags" else None
                head = (0, rows, cols, color.data_ptr(), var.data_ptr(), g.tri.data_ptr(), g.normal.data_ptr(), g.point.data_ptr(),
                        tp.P.ptr(al), None if prev_blk is None else C.byref(cam), tp.P.ptr(prev_blk), C.byref(par))
                tail = (nxt.data_ptr(), out.data_ptr(), out_v.data_ptr(), out_l.data_ptr())
                if how == "old":
                    tp.check(L.sq_temporal_accumulate_device(*head, *tail, None))
                else:
                    tp.check(L.sq_temporal_accumulate_moving_device(*head, None, 0, None, 0, None, 0, *tail, tp.P.ptr(flags), None))
                torch.cuda.synchronize()
                res.append((nxt, out, out_v, out_l))
            label = (rows, cols, prev_blk is not None, al is not None)
            assert all(same_exact(a, b) for a, b in zip(res[0], res[1])), label
            assert all(same_exact(a, b) for a, b in zip(res[0], res[2])), label + ("flags given",)
            want = M.accumulate(*cur, None if prev_blk is None else pcam, None if prev_blk is None else pwant,
                                alpha=None if al is None else alpha_host, sigma_p=SIGMA_P)
            assert np.array_equal(flags.cpu().numpy(), want["flags"]), label + ("flags",)


def test_python_layer_refusals(sqt, torch, tp):
    cur, _, _ = frames_for(5, 7, 1)
    color, var, g = gpu_frame(torch, cur)
    blk = tp.history(5, 7, 0)
    objects, back = M.tables(N_TRIS, 7)
    ot, bt = dev(torch, objects), dev(torch, back)
    E = tp.N.SquiglyError
    with pytest.raises(E, match="go together"):
        tp.accumulate(color, var, g, None, None, blk, objects=ot, sigma_p=SIGMA_P)
    with pytest.raises(E, match="go together"):
        tp.accumulate(color, var, g, None, None, blk, back=bt, sigma_p=SIGMA_P)
    with pytest.raises(E, match="objects must be"):
        tp.accumulate(color, var, g, None, None, blk, objects=ot.long(), back=bt, sigma_p=SIGMA_P)
    with pytest.raises(E, match="back must be"):
        tp.accumulate(color, var, g, None, None, blk, objects=ot, back=bt.reshape(-1), sigma_p=SIGMA_P)
    with pytest.raises(E, match="n_tris = 0"):
        tp.accumulate(color, var, g, None, None, blk, objects=ot[:0], back=bt, sigma_p=SIGMA_P)
    with pytest.raises(E, match="radius"):
        tp.accumulate(color, var, g, None, None, blk, clamp=(1.0, 4), sigma_p=SIGMA_P)
    with pytest.raises(E, match="form must be"):
        tp.accumulate(color, var, g, None, None, blk, clamp=1.0, form="lds", sigma_p=SIGMA_P)
    with pytest.raises(E, match="d_color and d_out overlap"):
        tp.accumulate(color, var, g, None, None, blk, clamp=1.0, out=(color, var), sigma_p=SIGMA_P)
    before = blk.clone()
    with pytest.raises(E, match="d_tri and d_object overlap"):
        tp.accumulate(color, var, g, None, None, blk, objects=g.tri.view(-1)[:N_TRIS], back=bt, sigma_p=SIGMA_P)
    torch.cuda.synchronize()
    assert torch.equal(blk, before)                                    # a refused call writes nothing


# ---- the driver, on the moving room ----
@pytest.fixture(scope="module")
def moving(sqt, torch, product_scene):
    """The moving room's mesh and poses, and a DeviceScene for each of its first three frames."""
    mesh, poses, box = MR.product_mesh(sqt, product_scene[2])
    scenes = [sqt.DeviceScene(sqt.BIH(sqt.moved_mesh(mesh, poses[f])), 0) for f in range(3)]
    yield mesh, poses, box, scenes
    torch.cuda.synchronize()
    for ds in scenes:
        ds.close()


def by_hand(torch, tp, ds, cam, prev_cam, prev, nxt, f, spp, period, params, back, clamp):
    """A Temporal.step with a scene written out in the primitive calls."""
    w, h = MR.W, MR.H
    denoise = importlib.import_module("squigly-trace_amd.denoise")
    sums = torch.zeros((w, h, 3), dtype=torch.float32, device="cuda")
    sums2 = torch.zeros((w, h, 3), dtype=torch.float32, device="cuda")
    k0 = (f % period) * spp
    ds.render_rows_masked(cam, spp * period, w, h, k0, k0 + spp, sums, sums2=sums2, want_avg=False, want_rgb=False)
    noisy = sums / float(spp)
    var = denoise.denoise_variance(sums, sums2, torch.full((w, h), spp, dtype=torch.int32, device="cuda"))
    g = ds.guides(cam, w, h)
    ok = ((g.tri >= 0) & (g.surf > 0).all(-1))[..., None]
    x = torch.where(ok, (noisy - g.emit) / torch.where(ok, g.surf, torch.ones_like(g.surf)), noisy)
    ls = (0.25 * g.surf[..., 0] + 0.5 * g.surf[..., 1]) + 0.25 * g.surf[..., 2]
    scale = torch.where(ok[..., 0], ls * ls, torch.ones_like(ls))
    kw = {} if back is None else dict(objects=torch.from_numpy(np.ascontiguousarray(ds.bih.tris["mat"], dtype=np.int32)).cuda(), back=back)
    out, out_var, length, flags = tp.accumulate(x, var / scale, g, prev_cam, prev, nxt, alpha=tp.frame_alpha(ds, g.tri), clamp=clamp,
                                                want_flags=True, **kw, **params)
    return torch.where(ok, out * g.surf + g.emit, out), out_var * scale, length, flags, g


def test_step_with_a_scene_is_the_primitive_calls(sqt, torch, tp, moving):
    """Three steps of sqt.Temporal, each on its own frame's scene with the move from the frame before and under a clamp, against
    the same primitive calls made by hand, bit for bit; the box's pixels are flagged as moved and keep their history."""
    mesh, poses, box, scenes = moving
    spp, period, clamp = 4, 3, (1.0, 2)
    cam = sqt.camera_from_text(MR.CAMERA_TEXT)
    sp = importlib.import_module("squigly-trace_amd.denoise").default_sigma_p(scenes[0].bih.bounds)
    params = dict(alpha_min=0.2, max_history=4, cos_n=0.9, sigma_p=sp)
    t = sqt.Temporal(scenes[0], MR.W, MR.H, spp, period=period, alpha_min=0.2, max_history=4, clamp=clamp)
    assert t.clamp == clamp and t.flags is None
    blocks = [tp.history(MR.W, MR.H, 0), tp.history(MR.W, MR.H, 0)]
    prev, prev_cam = None, None
    for f, ds in enumerate(scenes):
        back = None if f == 0 else tp.back_transforms(poses[f - 1], poses[f])
        avg, var, length, rgb = t.step(cam, scene=ds, back=back)
        want = by_hand(torch, tp, ds, cam, prev_cam, prev, blocks[f & 1], f, spp, period, params, back, clamp)
        torch.cuda.synchronize()
        assert same_exact((avg, var, length, t.flags), want[:4]), f
        assert same_exact(t.history, blocks[f & 1]) and t.frames == f + 1
        prev, prev_cam = blocks[f & 1], cam
    g = want[4]
    on_box = (g.tri >= 0) & (tp.object_table(scenes[2])[g.tri.clamp(min=0).long()] == box)
    assert int(on_box.sum()) >= 20
    assert bool(((t.flags[on_box] & tp.FLAG_MOVED) != 0).all()) and int(length[on_box].max()) == 3
    assert bool(((t.flags[g.tri >= 0] & tp.FLAG_MOVED) != 0).all())                    # (identity rows: the room's pixels go through B too)
    assert tp.object_table(scenes[2]) is tp.object_table(scenes[2])                     # cached per scene
    # without the move the box's pixels of the third frame find what used to be there: a shorter history
    t2 = sqt.Temporal(scenes[0], MR.W, MR.H, spp, period=period, alpha_min=0.2, max_history=4)
    for ds in scenes:
        _, _, length2, _ = t2.step(cam, scene=ds)
    torch.cuda.synchronize()
    assert t2.flags is None and float(length2[on_box].float().mean()) < float(length[on_box].float().mean())
    # what a step refuses of its scene
    E = sqt.SquiglyError
    with pytest.raises(E, match="back must have shape"):
        t.step(cam, scene=scenes[0], back=np.zeros((2, 12), f32))
    room = sqt.DeviceScene(sqt.BIH(sqt.Mesh.from_obj(os.path.join(DATA, "scene.obj"), DATA)), 0)
    try:
        with pytest.raises(E, match="materials"):
            t.step(cam, scene=room)
        scenes[1].set_depth(2)
        try:
            with pytest.raises(E, match="begun under"):
                t.step(cam, scene=scenes[1])
        finally:
            scenes[1].set_depth(3)
        with pytest.raises(E, match="sparse"):
            sqt.Temporal(scenes[0], MR.W, MR.H, spp, sparse=2).step(cam, scene=scenes[1])
    finally:
        torch.cuda.synchronize()
        room.close()


def read_png(path):
    """The (rows, cols, 3) uint8 image of a PNG as squigly-trace_amd.png writes it: 8-bit RGB, one IDAT, filter 0 on every row."""
    import struct
    import zlib
    raw = open(path, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks = 8, {}
    while at < len(raw):
        size, tag = struct.unpack(">I4s", raw[at:at + 8])
        chunks[tag] = raw[at + 8:at + 8 + size]
        at += 12 + size
    cols, rows, depth, kind = struct.unpack(">IIBB", chunks[b"IHDR"][:10])
    assert (depth, kind) == (8, 2)
    lines = np.frombuffer(zlib.decompress(chunks[b"IDAT"]), np.uint8).reshape(rows, 1 + 3 * cols)
    assert not lines[:, 0].any()
    return lines[:, 1:].reshape(rows, cols, 3)


def test_render_moving_sequence_and_cli(sqt, torch, tp, moving, tmp_path, monkeypatch):
    """render_moving_sequence gives the frames of the loop made by hand (moved_mesh, BIH, DeviceScene, step), with either build; and
    the CLI, given the moving room as an OBJ file and the poses as a .npy file, writes the same frames."""
    mesh, poses, box, scenes = moving
    cam = sqt.camera_from_text(MR.CAMERA_TEXT)
    n, spp, clamp = 3, 4, (1.0, 1)
    t = sqt.Temporal(scenes[0], MR.W, MR.H, spp, clamp=clamp)
    want = []
    for f in range(n):
        rgb = t.step(cam, scene=scenes[f], back=None if f == 0 else tp.back_transforms(poses[f - 1], poses[f]))[3]
        want.append(rgb.cpu().numpy())
    render = importlib.import_module("squigly-trace_amd.render")
    for build in (None, "device"):
        got = list(render.render_moving_sequence(mesh, [cam] * n, poses[:n], spp, (MR.W, MR.H), clamp=clamp, build=build))
        assert len(got) == n and all(np.array_equal(a, b) for a, b in zip(got, want)), build
    plain = list(sqt.render_moving_sequence(mesh, [cam] * n, poses[:n], spp, (MR.W, MR.H), temporal=False))
    assert np.array_equal(plain[0], list(sqt.render_moving_sequence(mesh, [cam], poses[:1], spp, (MR.W, MR.H)))[0])
    assert not np.array_equal(plain[2], want[2])
    # the CLI: the room's OBJ with the box appended under a material of its own
    data = tmp_path / "data"
    data.mkdir()
    obj = open(os.path.join(DATA, "scene.obj")).read()
    n_verts = sum(1 for line in obj.splitlines() if line.startswith("v "))
    rest = MR.box_rest().reshape(36, 3)
    # (the loader swaps the file's second and third coordinate, and reads an object as: o, its v lines, usemtl, s, its f lines)
    lines = ["o Box"] + ["v %s %s %s" % tuple(repr(float(c)) for c in (v[0], v[2], v[1])) for v in rest] + ["usemtl Box", "s off"]
    lines += ["f %d %d %d" % (n_verts + 3 * i + 1, n_verts + 3 * i + 2, n_verts + 3 * i + 3) for i in range(12)]
    (data / "room.obj").write_text(obj.replace("mtllib scene.sq", "mtllib room.sq") + "\n".join(lines) + "\n")
    sq = open(os.path.join(DATA, "scene.sq")).read()
    (data / "room.sq").write_text(sq + "\nnewmtl Box\nreflective 0 %r %r %r\nemissive 0 0 0 0\n" % MR.BOX_SURF)
    cli = importlib.import_module("squigly-trace_amd.cli")
    loaded = sqt.Mesh.from_obj(str(data / "room.obj"), str(data))
    box_mat = int(loaded.tris["mat"][-1])
    assert len(loaded) == len(mesh) and len(loaded.materials) == len(mesh.materials)
    assert np.array_equal(np.array(loaded.tris), np.array(mesh.tris)) and box_mat == box
    cli_poses = np.tile(np.eye(3, 4), (n, len(loaded.materials), 1, 1))
    cli_poses[:, box_mat, 0, 3] = MR.STEP * np.arange(n)
    np.save(tmp_path / "poses.npy", cli_poses)
    (tmp_path / "still.cams").write_bytes(MR.CAMERA_TEXT * n)
    monkeypatch.chdir(tmp_path)
    path = tmp_path / "out" / "move.png"
    assert cli.main(["-s", str(spp), "-d", f"{MR.W},{MR.H}", "-p", str(path), "--objpath", str(data / "room.obj"), "--sequence",
                     str(tmp_path / "still.cams"), "--temporal", "--poses", str(tmp_path / "poses.npy"), "--history-clamp", "1,1"]) == 0
    by_cli = list(sqt.render_moving_sequence(loaded, [cam] * n, cli_poses, spp, (MR.W, MR.H), clamp=clamp))
    for p, img in zip(cli.view_paths(str(path), n), by_cli):
        assert np.array_equal(read_png(p), img), p
    # the loaded file is the same scene: the same frames as the mesh built from arrays, whatever the order of its materials
    assert all(np.array_equal(a, b) for a, b in zip(by_cli, want))
