"""Motion blur on the GPU (libsquigly_shutter.so, DeviceScene.shutter_rays / render_shutter / render_shutter_masked): the ray kernels
and whole frames equal tests/shutter_restatement.py (pinned to the oracle by tests/test_shutter.py) bit for bit with NaN = NaN; four
pins tie the library to the two lens libraries and to the main one without any restatement; the listed form, AdaptiveLens(motion=)
and the command line.  (The calls on a gated non-blocking stream are tests/test_gpu_streams_shutter.py.)"""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import depth_restatement as DR
import lens_restatement as LR
import mlens_restatement as MR
import shutter_restatement as SHR
import sky_restatement as SR
from bitcmp import ibits, nan_eq, same_exact
from conftest import DATA, ROOT
from masked_calls import SENT, buffers, host
from render_options import set_sky_options as set_options

pytestmark = pytest.mark.gpu
f32 = np.float32
W, H, S = SHR.W, SHR.H, SHR.S
P = W * H
JITTERS = [0.0, 0.5, 1.0]


class Room:
    pass


@pytest.fixture(scope="module")
def room(sqt):
    import torch
    r = Room()
    r.bright = DR.case("bright")                 # the room under materials that let most samples carry light: the frames' scene
    r.bds = sqt.DeviceScene(r.bright.bih, 0)
    r.lens = importlib.import_module("squigly-trace_amd.lens")
    r.shutter = importlib.import_module("squigly-trace_amd.shutter")
    r.shutter.lib()
    r.torch = torch
    yield r
    torch.cuda.synchronize()
    r.bds.close()


def motion(sqt, time_jitter=1.0, m=SHR.MOTION):
    return sqt.Motion((m[0], m[1]), (m[2], m[3]), time_jitter)


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def assert_rays(got, want, label):
    (o, d, s), (wo, wd, ws) = got, want
    o, d, s = (t.cpu().numpy() for t in (o, d, s))
    nb = wo.shape[0]
    assert o.shape[0] == nb and o.reshape(nb, -1, 3).shape == wo.shape
    for name, g, e in (("origins", o, wo), ("directions", d, wd)):
        ok = nan_eq(g.reshape(e.shape), e).all(-1)
        assert ok.all(), (label, name, int((~ok).sum()), np.argwhere(~ok)[:4])
    assert np.array_equal(s.reshape(ws.shape), ws), (label, "seeds")


def assert_frame(got, want, label):
    s, q, avg, rgb = want
    for name, g, e in (("sum", got.sum, s), ("sum2", got.sum2, q), ("avg", got.avg, avg)):
        ok = nan_eq(g.cpu().numpy().reshape(-1, 3), e).all(-1)
        assert ok.all(), (label, name, int((~ok).sum()), np.nonzero(~ok)[0][:6])
    assert np.array_equal(got.rgb.cpu().numpy().reshape(-1, 3), rgb), (label, "rgb")


def want_frame(lens_name, R, tj, depth=3, sky=None):
    parts = LR.sub_ray_sums(SHR.room_trails(lens_name, R, tj), depth, sky)
    s, q, avg = LR.fold(parts, S)
    return parts, (s, q, avg, LR.tonemap(avg))


# ---- 1. rays and frames against the restatement --------------------------------------------------------------------------
@pytest.mark.parametrize("tj", JITTERS)
@pytest.mark.parametrize("lens_name", list(SHR.LENSES))
@pytest.mark.parametrize("R", [1, 2, 4, 8])
def test_rays_and_frames_equal_the_restatement(sqt, room, R, lens_name, tj):
    set_options(room.bds)
    lens = sqt.Lens(*SHR.LENSES[lens_name])
    got = room.bds.shutter_rays(motion(sqt, tj), lens, S, R, W, H)
    want = SHR.room_rays(lens_name, R, tj)
    assert_rays(got, want, (R, lens_name, tj))
    if R > 1:                                    # the sub-rays of a pixel start from different poses
        assert (ibits(want[0][0]) != ibits(want[0][R - 1])).any(-1).all()
    parts, frame = want_frame(lens_name, R, tj)
    assert (frame[0] != 0).any(-1).sum() > 100
    assert_frame(room.bds.render_shutter(motion(sqt, tj), lens, S, R, W, H, want_sum2=True), frame, (R, lens_name, tj))


def test_rays_of_less_than_a_wave_of_a_range_and_of_a_shard(sqt, room):
    lens = SHR.LENSES["both"]
    m = motion(sqt, 0.5)
    got = room.bds.shutter_rays(m, sqt.Lens(*lens), 6, 3, 5, 7)
    assert got[0].shape == (3, 5, 7, 3) and got[2].shape == (3, 5, 7)
    want = SHR.rays(SHR.MOTION, 0.5, lens, 6, 3, 5, 7)
    assert_rays(got, want, "5 x 7")
    part = room.bds.shutter_rays(m, sqt.Lens(*lens), 6, 3, 5, 7, r_range=(1, 3))
    assert_rays(part, tuple(a[1:3] for a in want), "5 x 7, sub-rays 1 and 2")
    shard = (2, 1, 3)
    rows = DR.shard_rows(40, shard)
    got = room.bds.shutter_rays(m, sqt.Lens(*lens), 6, 2, 40, 72, shard=shard)
    assert got[0].shape == (2, len(rows), 72, 3)
    assert_rays(got, SHR.rays(SHR.MOTION, 0.5, lens, 6, 2, 40, 72, rows=rows), "40 x 72, shard 1 of 3")


def test_a_frame_at_depth_5_under_a_sky(sqt, room):
    try:
        set_options(room.bds, sky=SR.GRADIENT, depth=5)
        _, frame = want_frame("both", 8, 1.0, 5, SR.GRADIENT)
        got = room.bds.render_shutter(motion(sqt), sqt.Lens(*SHR.LENSES["both"]), S, 8, W, H, want_sum2=True)
        assert_frame(got, frame, "depth 5 under a sky")
        assert not nan_eq(frame[0], want_frame("both", 8, 1.0)[1][0]).all()
    finally:
        set_options(room.bds)


# ---- 2. the four pins ------------------------------------------------------------------------------------------------------
def full_list(room):
    index, n_live = room.bds.live_pixels(cuda(np.ones((W, H), np.uint8)), None, 0)
    assert int(n_live.item()) == P
    return index


@pytest.mark.parametrize("tj", JITTERS)
def test_pin_1_equal_poses_are_the_lens_libraries_frames(sqt, room, tj):
    set_options(room.bds)
    still = motion(sqt, tj, SHR.STILL)
    cam = still.pose(0)
    assert bytes(cam) == bytes(sqt.load_camera(os.path.join(DATA, "camera")))
    for lens_name in ("both", "plain"):
        lens = sqt.Lens(*SHR.LENSES[lens_name])
        want = room.bds.render_lens(cam, lens, S, 4, W, H, want_sum2=True)
        assert (want.sum != 0).any()
        got = room.bds.render_shutter(still, lens, S, 4, W, H, want_sum2=True)
        assert same_exact(tuple(got), tuple(want)), (lens_name, tj)
        assert same_exact(room.bds.shutter_rays(still, lens, S, 4, W, H), room.bds.lens_rays(cam, lens, S, 4, W, H))
        # listed: a mask, two ranges, against sq_mlens_render_device
        rng = np.random.default_rng(41)
        mask = cuda((rng.random((W, H)) < 0.4).astype(np.uint8))
        A, B = buffers(W, H), buffers(W, H)
        for r0, r1 in ((0, 3), (3, 4)):
            index, n_live = room.bds.live_pixels(mask, A["counts"], r0)
            n = int(n_live.item())
            assert 100 < n < 200
            room.bds.render_lens_masked(cam, lens, S, 4, W, H, r0, r1, A["sums"], index, n, sums2=A["sums2"], counts=A["counts"], out_avg=A["avg"],
                                        out_rgb=A["rgb"])
            room.bds.render_shutter_masked(still, lens, S, 4, W, H, r0, r1, B["sums"], index, n, sums2=B["sums2"], counts=B["counts"],
                                           out_avg=B["avg"], out_rgb=B["rgb"])
            assert same_exact(tuple(B.values()), tuple(A.values())), (lens_name, tj, r0)


@pytest.mark.parametrize("R", [1, 2, 4, 8])
def test_pin_2_without_time_jitter_a_sub_ray_is_lens_rays_under_its_pose(sqt, room, R):
    m = motion(sqt, 0.0)
    for lens_name in SHR.LENSES:
        lens = sqt.Lens(*SHR.LENSES[lens_name])
        got = room.bds.shutter_rays(m, lens, S, R, W, H)
        for r in range(R):
            want = room.bds.lens_rays(m.pose(r / R), lens, S, R, W, H, r_range=(r, r + 1))
            assert same_exact(tuple(t[r] for t in got), tuple(t[0] for t in want)), (R, lens_name, r)
    if R > 1:
        assert not same_exact(got[0][0], got[0][R - 1])


def test_pin_3_one_plain_sub_ray_is_the_main_librarys_frame(sqt, room):
    set_options(room.bds)
    m = motion(sqt, 0.0)
    got = room.bds.render_shutter(m, sqt.Lens(jitter=0), 4, 1, 64, 64)
    avg, rgb = room.bds.render_rows(m.pose(0), 4, 64, 64)
    assert same_exact(got.avg, avg) and same_exact(got.rgb, rgb) and (avg != 0).any()
    try:                                         # and of a shard, under a depth and a sky
        set_options(room.bds, sky=SR.GRADIENT, depth=4)
        got = room.bds.render_shutter(m, sqt.Lens(jitter=0), 3, 1, 40, 72, shard=(2, 1, 3))
        avg, rgb = room.bds.render_rows(m.pose(0), 3, 40, 72, shard=(2, 1, 3))
        assert same_exact(got.avg, avg) and same_exact(got.rgb, rgb)
    finally:
        set_options(room.bds)


def test_pin_4_ranges_batches_and_shards_give_one_calls_bits(sqt, room):
    set_options(room.bds)
    m, lens = motion(sqt), sqt.Lens(*SHR.LENSES["both"])
    whole = room.bds.render_shutter(m, lens, S, 8, W, H, want_sum2=True)
    assert (whole.sum != 0).any()
    # the ranges (0, 3) and (3, 8)
    first = room.bds.render_shutter(m, lens, S, 8, W, H, r_range=(0, 3), want_sum2=True)
    rest = room.bds.render_shutter(m, lens, S, 8, W, H, r_range=(3, 8), sums=(first.sum, first.sum2))
    assert rest.sum is first.sum and same_exact(tuple(rest), tuple(whole))
    # a workspace of one sub-ray: eight batches
    nbytes = room.lens.work_bytes(P, 1)
    assert len(room.lens.plan(P, 0, 8, nbytes)) == 8
    assert same_exact(tuple(room.bds.render_shutter(m, lens, S, 8, W, H, want_sum2=True, work_mb=nbytes / 2 ** 20)), tuple(whole))
    # three shards of row_block 2
    seen = np.zeros(W, bool)
    for k in range(3):
        rows = DR.shard_rows(W, (2, k, 3))
        part = room.bds.render_shutter(m, lens, S, 8, W, H, shard=(2, k, 3), want_sum2=True)
        assert part.sum.shape == (len(rows), H, 3)
        assert same_exact(tuple(part), tuple(t[list(rows)] for t in whole)), k
        seen[list(rows)] = True
    assert seen.all()


# ---- 3. the listed form -----------------------------------------------------------------------------------------------------
def masked_shutter(room, m, lens, R, r0, r1, B, mask, work_mb=None):
    index, n_live = room.bds.live_pixels(None if mask is None else cuda(np.ascontiguousarray(mask, np.uint8).reshape(W, H)), B["counts"], r0)
    n = int(n_live.item())
    room.bds.render_shutter_masked(m, lens, S, R, W, H, r0, r1, B["sums"], index, n, sums2=B["sums2"], counts=B["counts"], work_mb=work_mb,
                                   out_avg=B["avg"], out_rgb=B["rgb"])
    room.torch.cuda.synchronize()
    return n


def fresh_state():
    return {"sum": np.full((P, 3), SENT["sums"], f32), "sum2": np.full((P, 3), SENT["sums2"], f32), "count": np.full(P, SENT["counts"], np.int32),
            "avg": np.full((P, 3), SENT["avg"], f32), "rgb": np.full((P, 3), SENT["rgb"], np.uint8)}


def assert_buffers(B, st, label):
    b = host(B)
    for k, name in (("sum", "sums"), ("sum2", "sums2"), ("avg", "avg")):
        ok = nan_eq(b[name].reshape(-1, 3), st[k]).all(-1)
        assert ok.all(), (label, name, int((~ok).sum()), np.nonzero(~ok)[0][:6])
    assert np.array_equal(b["counts"].reshape(-1), st["count"]) and np.array_equal(b["rgb"].reshape(-1, 3), st["rgb"]), label


def test_listed_frames_equal_the_restatement(sqt, room):
    """A checkerboard in one call, and a random mask that shrinks between two ranges (the counts guard the gap): the listed pixels
    hold the restatement's fold with the pixel's own divisor, and the sentinels of every other pixel are untouched."""
    set_options(room.bds)
    m, lens = motion(sqt), sqt.Lens(*SHR.LENSES["both"])
    parts, _ = want_frame("both", 8, 1.0)
    checker = (np.add.outer(np.arange(W), np.arange(H)) % 2).astype(np.uint8)
    B = buffers(W, H)
    assert masked_shutter(room, m, lens, 8, 0, 8, B, checker) == P // 2
    st = fresh_state()
    idx = MR.live_list(checker.reshape(-1), None, 0)
    MR.indexed_fold(parts[:, idx], idx, 1, 0, 8, st)
    assert_buffers(B, st, "checkerboard")
    assert (st["sum"][idx] != 0).any(-1).sum() > 40 and (st["count"] == SENT["counts"]).sum() == P // 2
    # a random mask, then a shrunken one whose first pixel has a count that does not match
    rng = np.random.default_rng(43)
    mask1 = (rng.random((W, H)) < 0.3).astype(np.uint8)
    mask2 = mask1 & (rng.random((W, H)) < 0.6).astype(np.uint8)
    B, st = buffers(W, H), fresh_state()
    n1 = masked_shutter(room, m, lens, 8, 0, 3, B, mask1)
    idx1 = MR.live_list(mask1.reshape(-1), None, 0)
    assert n1 == len(idx1)
    MR.indexed_fold(parts[0:3][:, idx1], idx1, 1, 0, 3, st)
    assert_buffers(B, st, "first range")
    gap = int(np.flatnonzero(mask2.reshape(-1))[0])
    B["counts"].view(-1)[gap] = 2
    st["count"][gap] = 2
    nbytes = room.lens.work_bytes(int(mask2.sum()) - 1, 2)
    n2 = masked_shutter(room, m, lens, 8, 3, 8, B, mask2, work_mb=nbytes / 2 ** 20)             # three batches
    idx2 = MR.live_list(mask2.reshape(-1), st["count"], 3)
    assert n2 == len(idx2) == int(mask2.sum()) - 1
    MR.indexed_fold(parts[3:8][:, idx2], idx2, 1, 3, 8, st)
    assert_buffers(B, st, "second range")
    assert set(np.unique(st["count"])) == {2, 3, 8, SENT["counts"]}


def test_a_list_with_entries_out_of_range(sqt, room):
    """Entries outside [0, P) give a ray of zeros and are skipped by the fold: every other listed pixel is right, nothing else is written."""
    set_options(room.bds)
    torch, L = room.torch, room.shutter.lib()
    m, lens = motion(sqt), sqt.Lens(*SHR.LENSES["both"])
    good = np.arange(5, P, 7, dtype=np.int32)
    entries = np.concatenate([[-1], good[:20], [P, 2 ** 31 - 1], good[20:], [-2 ** 31]]).astype(np.int32)
    index = cuda(entries)
    n = len(entries)
    sh = sqt.Shard(W, 0, 1)
    o = torch.full((2, n, 3), 9.0, dtype=torch.float32, device="cuda:0")
    d = torch.full((2, n, 3), 9.0, dtype=torch.float32, device="cuda:0")
    sd = torch.full((2, n), 9, dtype=torch.int64, device="cuda:0")
    room.shutter.check(L.sq_shutter_rays_device(0, C.byref(m), C.byref(lens), S, 8, 2, 4, W, H, sh, index.data_ptr(), n, o.data_ptr(), d.data_ptr(),
                                                sd.data_ptr(), None))
    torch.cuda.synchronize()
    ro, rd, rs = SHR.room_rays("both", 8, 1.0)
    ok = (entries >= 0) & (entries < P)
    o, d, sd = o.cpu().numpy(), d.cpu().numpy(), sd.cpu().numpy()
    assert nan_eq(o[:, ok], ro[2:4][:, good]).all() and nan_eq(d[:, ok], rd[2:4][:, good]).all() and np.array_equal(sd[:, ok], rs[2:4][:, good])
    assert (ibits(o[:, ~ok]) == 0).all() and (ibits(d[:, ~ok]) == 0).all() and (sd[:, ~ok] == 0).all()
    B = buffers(W, H)
    nbytes = room.lens.work_bytes(n, 8)
    work = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
    room.shutter.check(L.sq_shutter_render_device(room.bds._h, C.byref(m), C.byref(lens), S, 8, 0, 8, W, H, sh, index.data_ptr(), n, work.data_ptr(), nbytes,
                                                  B["sums"].data_ptr(), B["sums2"].data_ptr(), B["counts"].data_ptr(), B["avg"].data_ptr(),
                                                  B["rgb"].data_ptr(), None))
    torch.cuda.synchronize()
    parts, _ = want_frame("both", 8, 1.0)
    st = fresh_state()
    MR.indexed_fold(parts[:, good], good, 1, 0, 8, st)
    assert_buffers(B, st, "a list with entries out of range")


# ---- 4. AdaptiveLens(motion=) ------------------------------------------------------------------------------------------------
def test_adaptive_lens_under_a_motion(sqt, room):
    """Two steps equal the masked calls made by hand; a checkpoint resumes to the same bits; a resume under another motion, or under
    none, is refused."""
    set_options(room.bds)
    m, lens = motion(sqt), sqt.Lens(*SHR.LENSES["aa"])
    cam = m.pose(0)
    a = sqt.AdaptiveLens(room.bds, cam, lens, S, 8, W, H, MR.TOL, eps=1e-3, first=2, step=2, motion=m)
    assert a.motion is m and a.live == P
    B = buffers(W, H)
    mask = np.ones((W, H), np.uint8)
    ckpt = None
    for step, (r0, r1) in enumerate(((0, 2), (2, 4))):
        avg, rgb = a.step()
        assert masked_shutter(room, m, lens, 8, r0, r1, B, mask) == (P if step == 0 else int(mask.sum()))
        b = host(B)
        mask = sqt.rule_reference(b["sums"], b["sums2"], b["counts"], mask, MR.TOL, 1e-3)
        live = mask != 0
        assert same_exact((a.sums, a.sums2), (B["sums"], B["sums2"])) and same_exact(a.mask, cuda(mask.astype(np.uint8)))
        assert same_exact((avg, rgb), (B["avg"], B["rgb"])) and (a.counts.cpu().numpy() == b["counts"]).all()
        assert a.live == int(live.sum()) and a.done == r1
        if step == 0:
            assert 20 < a.live < P                       # the rule stopped some pixels, so the second step runs on a true list
            ckpt = dict(sums=a.sums.cpu().numpy(), sums2=a.sums2.cpu().numpy(), counts=a.counts.cpu().numpy(), mask=a.mask.cpu().numpy(),
                        done=a.done, depth=a.depth, sky=a.sky, motion=a.motion)
    # the frame is not the static one's
    static = sqt.AdaptiveLens(room.bds, cam, lens, S, 8, W, H, MR.TOL, eps=1e-3, first=2, step=2)
    assert static.motion is None
    static.step()
    assert not same_exact(static.sums, cuda(ckpt["sums"]))
    # resumed after step 1 under the checkpoint's motion (an equal one, compared by bits): the same bits after step 2
    again = motion(sqt)
    b2 = sqt.AdaptiveLens(room.bds, cam, lens, S, 8, W, H, MR.TOL, eps=1e-3, first=2, step=2, checkpoint_motion=again, **ckpt)
    assert b2.done == 2
    avg_b, rgb_b = b2.step()
    assert same_exact((b2.sums, b2.sums2, b2.counts, b2.mask, avg_b, rgb_b), (a.sums, a.sums2, a.counts, a.mask, avg, rgb))
    for other in (motion(sqt, 0.5), motion(sqt, 1.0, SHR.STILL), None):
        with pytest.raises(sqt.SquiglyError, match="motion"):
            sqt.AdaptiveLens(room.bds, cam, lens, S, 8, W, H, MR.TOL, eps=1e-3, first=2, step=2, checkpoint_motion=other, **ckpt)
    with pytest.raises(sqt.SquiglyError, match="motion"):
        sqt.AdaptiveLens(room.bds, cam, lens, S, 8, W, H, MR.TOL, eps=1e-3, first=2, step=2, checkpoint_motion=m, **{**ckpt, "motion": None})


# ---- 5. the blur is there ------------------------------------------------------------------------------------------------------
def test_the_moving_frame_differs_from_both_static_frames(sqt, room):
    """Among the pixels whose plain ray hits the scene at some instant (the CPU oracle's first hits at tt = 0, 0.25, 0.5, 0.75, 1), the
    moving frame's avg differs from the static frame's at pose(0) and at pose(1) on at least a quarter each."""
    set_options(room.bds)
    m, lens = motion(sqt), sqt.Lens(*SHR.LENSES["aa"])
    hit = np.zeros(P, bool)
    for tt in (0.0, 0.25, 0.5, 0.75, 1.0):
        hit |= SHR.first_hits_at(room.bright.ob, SHR.MOTION, tt) >= 0
    assert hit.sum() >= 150
    moving = ibits(room.bds.render_shutter(m, lens, S, 8, W, H).avg).reshape(P, 3)
    for tt in (0.0, 1.0):
        static = ibits(room.bds.render_lens(m.pose(tt), lens, S, 8, W, H).avg).reshape(P, 3)
        share = float((moving != static).any(-1)[hit].mean())
        print(f"moving frame against the static frame at pose({tt:g}): differs on {share:.3f} of {int(hit.sum())} hit pixels")
        assert share >= 0.25, (tt, share)


# ---- 6. refusals on the device, and the command line ------------------------------------------------------------------------------
def test_refusals_leave_every_buffer_as_it_was(sqt, room):
    torch, L = room.torch, room.shutter.lib()
    set_options(room.bds)
    B = buffers(W, H)
    nbytes = room.lens.work_bytes(P, 8)
    work = torch.full((nbytes + 64,), 0x3C, dtype=torch.uint8, device="cuda:0")
    index = full_list(room)
    keep = index.clone()
    sh = sqt.Shard(W, 0, 1)

    def call(scene=room.bds._h, tj=1.0, lens=(1.0, 0.0, 1.0), R=4, r=(0, 4), listed=False, n=P, work_ptr=None, work_bytes=nbytes, **ptr):
        a = {"sum": B["sums"].data_ptr(), "sum2": B["sums2"].data_ptr(), "count": B["counts"].data_ptr() if listed else None,
             "avg": B["avg"].data_ptr(), "rgb": B["rgb"].data_ptr(), **ptr}
        ln = room.lens.Lens.__new__(room.lens.Lens)
        C.Structure.__init__(ln, *lens)
        m = motion(sqt)
        m.time_jitter = tj
        rc = L.sq_shutter_render_device(scene, C.byref(m), C.byref(ln), S, R, r[0], r[1], W, H, sh, index.data_ptr() if listed else None, n,
                                        work.data_ptr() if work_ptr is None else work_ptr, work_bytes, a["sum"], a["sum2"], a["count"], a["avg"],
                                        a["rgb"], None)
        return rc, L.sq_shutter_last_error().decode()

    cases = [(dict(scene=None), "null argument"), (dict(sum=None), "null argument"), (dict(R=3), "must divide"), (dict(r=(0, 5)), "bad sub-ray range"),
             (dict(tj=1.5), "time_jitter"), (dict(tj=float("nan")), "time_jitter"), (dict(lens=(1.5, 0.0, 1.0)), "jitter"),
             (dict(lens=(1.0, 0.1, 0.0)), "focus"), (dict(count=B["counts"].data_ptr()), "d_count needs a list"),
             (dict(listed=True, n=P + 1), "the list must hold"), (dict(work_bytes=room.lens.work_bytes(P, 1) - 1), "too small"),
             (dict(work_ptr=work.data_ptr() + 8), "16-byte aligned"), (dict(sum2=B["sums"].data_ptr() + 12), "d_sum and d_sum2 overlap"),
             (dict(rgb=work.data_ptr() + 16), "d_rgb and d_work overlap"), (dict(listed=True, avg=index.data_ptr()), "d_index and d_avg overlap")]
    for kw, message in cases:
        rc, err = call(**kw)
        assert rc != 0 and message in err, (kw, err)
    o = torch.full((4, P, 3), 9.0, dtype=torch.float32, device="cuda:0")
    sd = torch.full((4, P), 9, dtype=torch.int64, device="cuda:0")
    m, ln = motion(sqt), sqt.Lens()
    assert L.sq_shutter_rays_device(0, C.byref(m), C.byref(ln), S, 4, 0, 4, W, H, sh, None, 0, o.data_ptr(), o.data_ptr() + 12, sd.data_ptr(), None) != 0
    assert "d_org and d_dir overlap" in L.sq_shutter_last_error().decode()
    with pytest.raises(sqt.SquiglyError, match="too small"):
        room.bds.render_shutter(m, ln, S, 4, W, H, work_mb=1e-3)
    torch.cuda.synchronize()
    b = host(B)
    assert all((b[k] == SENT[k]).all() for k in ("sums", "sums2", "counts", "avg", "rgb"))
    assert (work == 0x3C).all() and (o == 9.0).all() and (sd == 9).all() and torch.equal(index, keep)


def test_cli_shutter_camera_frame_is_render_shutter(sqt, room, tmp_path, monkeypatch):
    from PIL import Image
    cli = importlib.import_module("squigly-trace_amd.cli")
    monkeypatch.chdir(ROOT)                                          # the reference's default obj and camera paths are relative
    close = tmp_path / "close"
    p1, a1 = (tuple(float(f32(v)) for v in part) for part in SHR.CLOSE)
    close.write_text(" ".join(f"{v:.30f}" for v in p1) + "\n" + " ".join(f"{v:.30f}" for v in a1) + "\n")
    opened = open(os.path.join(DATA, "camera"), "rb").read()
    assert bytes(sqt.Motion(opened, close.read_bytes())) == bytes(motion(sqt))           # the texts give the test motion's bits
    ds = sqt.DeviceScene(LR.room()[0].bih, 0)
    try:
        out = str(tmp_path / "blur.png")
        assert cli.main(["-s", "8", "-d", "24,32", "-p", out, "--shutter-camera", str(close), "--aa", "--subrays", "4"]) == 0
        want = ds.render_shutter(motion(sqt), sqt.Lens(), 8, 4, 24, 32).rgb.cpu().numpy()
        assert np.array_equal(np.array(Image.open(out).convert("RGB")), want) and want.any()
        # alone: Lens(jitter=0), a ray per sample; with its jitter, a depth and a sky
        out2 = str(tmp_path / "blur2.png")
        assert cli.main(["-s", "4", "-d", "24,32", "-p", out2, "--shutter-camera", str(close), "--shutter-jitter", "0.5", "--depth", "2",
                         "--sky", "0.5,0.5,1"]) == 0
        set_options(ds, sky=((0.5, 0.5, 1.0), (0.5, 0.5, 1.0)), depth=2)
        want2 = ds.render_shutter(motion(sqt, 0.5), sqt.Lens(jitter=0), 4, 4, 24, 32).rgb.cpu().numpy()
        set_options(ds)
        assert np.array_equal(np.array(Image.open(out2).convert("RGB")), want2)
        assert np.array_equal(sqt.render_lens_rgb8(LR.room()[0].bih, None, 8, (24, 32), subrays=4, motion=motion(sqt)), want)
    finally:
        ds.close()
