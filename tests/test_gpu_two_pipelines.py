"""The automatic schedule on the GPU: two pipelines chosen by the planner, here with the mirror rays at the head of batch 0's first
trace launch (option "mirror_ride" = 1; the library's default gives them a launch of their own, which one test below holds to the same
frame) (csrc/sq_plan_call.h: plan_schedule; csrc/sq_device.hip: launch_frame).

Option "auto_overlap_slots" = 1 makes the small frames below take the schedule that large frames take by default.  Every call is
compared bit for bit with the same call under "auto_overlap" = 0, the serial schedule: avg, RGB8, the fold, second moments and
counts where the call has them, and the counters 0 (rays traced) and 28-30 (first-bounce rays level-1 culling dropped).  The trace
launches that option "timing" counts show that the schedule under test is the one that ran and that the mirror rays rode: two per
batch and none besides.  Two shapes are held to the committed golden frames as well, and one call runs on a gated side stream
(tests/stream_harness.py): the default path now uses the scene's second stream."""
import os

import numpy as np
import pytest

import masked_calls as MC
import render_options as RO
import stream_harness as SH
from bitcmp import ibits
from conftest import DATA, GOLDEN
from scenes import ROTATED

pytestmark = pytest.mark.gpu
MISS = b"0 7 0.75\n-1.5707963267948966 0 0\n"          # looks away from the scene: every primary ray misses
STAT_SLOTS = (0, 28, 29, 30)
AUTO = {"auto_overlap": 1, "auto_overlap_slots": 1, "mirror_ride": 1}
SERIAL = {"auto_overlap": 0, "auto_overlap_slots": 1, "mirror_ride": 1}
DEFAULTS = {**RO.FRAME, "auto_overlap": 1, "auto_overlap_slots": 1 << 26, "batches_per_track": 1, "mirror_ride": 0}


@pytest.fixture
def dev(sqt, product_scene):
    """A fresh scene per test: its workspace holds the slots the test's own calls want and no more (a workspace only grows, and the
    batches follow the slots it has), so the launch counts below are those of the planner's rule."""
    assert sqt.device_count() >= 1, "no HIP device: the product has no CPU fallback"
    ds = sqt.DeviceScene(product_scene[0], 0)
    yield ds
    ds.close()


def cam_of(sqt, text=None):
    return sqt.camera_from_text(open(os.path.join(DATA, "camera"), "rb").read() if text is None else text)


def frame_call(w, h, n, text=None, shard=(None, 0, 1)):
    def call(sqt, ds):
        a, r = ds.render_rows(cam_of(sqt, text), n, w, h, shard=shard)
        return {"avg": a, "rgb": r}
    return call


def range_call(w, h, n, k0, k1):
    """[0, k0) under the serial schedule in both runs, then [k0, k1) under the schedule in force."""
    def call(sqt, ds):
        import torch
        sums = torch.zeros((w, h, 3), dtype=torch.float32, device="cuda:0")
        now = {k: v for k, v in (AUTO if call.auto else SERIAL).items()}
        RO.set_options(ds, SERIAL)
        ds.render_rows_range(cam_of(sqt), n, w, h, 0, k0, sums)
        torch.cuda.synchronize()
        ds.stats(reset=True)
        ds.reset_timing()
        RO.set_options(ds, now)
        a, r = ds.render_rows_range(cam_of(sqt), n, w, h, k0, k1, sums)
        return {"avg": a, "rgb": r, "sums": sums}
    call.auto = False
    return call


def masked_call(w, h, n):
    def call(sqt, ds):
        B = MC.buffers(w, h)
        y, x = np.indices((w, h))
        MC.masked(ds, cam_of(sqt), n, w, h, 0, n, B, ((y + x) % 3 != 0).astype(np.uint8))
        return B
    return call


def views_call(w, h, n):
    def call(sqt, ds):
        a, r = ds.render_views([cam_of(sqt), cam_of(sqt, ROTATED)], n, w, h)
        return {"avg": a, "rgb": r}
    return call


# name -> (the call, options besides the schedule's, trace launches of the automatic schedule = 2 x its batches)
CASES = {
    "8x8@2 one sample per track": (frame_call(8, 8, 2), {}, 4),
    "8x8@3 odd tail": (frame_call(8, 8, 3), {}, 6),
    "8x8@5 slots 128, five batches": (frame_call(8, 8, 5), {"slots": 128}, 10),
    "40x72@3": (frame_call(40, 72, 3), {}, 6),
    "8x8@9 batches of four and a ragged one": (frame_call(8, 8, 9), {}, 6),
    "every primary ray misses": (frame_call(8, 8, 4, MISS), {}, 4),
    "resident 0": (frame_call(8, 8, 4), {"resident": 0}, 4),
    "masked with second moments": (masked_call(9, 13, 4), {}, 4),
    "two views": (views_call(8, 8, 4), {}, 4),
    "samples 3..7": (range_call(8, 8, 7, 3, 7), {}, 4),
    "shard (2, 1, 2) of 40x72@3": (frame_call(40, 72, 3, shard=(2, 1, 2)), {}, 6),
}
GOLDEN_ROWS = {"40x72@3": slice(None), "shard (2, 1, 2) of 40x72@3": [r for r in range(40) if (r // 2) % 2 == 1]}


def run(sqt, torch, ds, call, schedule, opts):
    """The call under a schedule: ({name: numpy} of its outputs, the four counters, trace launches)."""
    RO.set_options(ds, DEFAULTS, **schedule, **opts)
    if hasattr(call, "auto"):
        call.auto = schedule is AUTO
    torch.cuda.synchronize()
    ds.stats(reset=True)
    ds.reset_timing()
    ds.enable_timing(True)
    try:
        out = call(sqt, ds)
        torch.cuda.synchronize()
        launches = ds.kernel_timing()[1]
    finally:
        ds.enable_timing(False)
        ds.reset_timing()
    st = ds.stats(reset=True)
    RO.set_options(ds, DEFAULTS)
    return {k: v.cpu().numpy() for k, v in out.items()}, [st[i] for i in STAT_SLOTS], launches


@pytest.mark.parametrize("name", list(CASES))
def test_automatic_schedule_equals_the_serial_one(sqt, dev, name):
    import torch
    call, opts, want_launches = CASES[name]
    serial, serial_stats, serial_launches = run(sqt, torch, dev, call, SERIAL, opts)
    auto, auto_stats, auto_launches = run(sqt, torch, dev, call, AUTO, opts)
    print(f"{name}: trace launches serial {serial_launches}, automatic {auto_launches}; counters {auto_stats}")
    assert set(auto) == set(serial)
    for k in serial:
        assert auto[k].dtype == serial[k].dtype and auto[k].shape == serial[k].shape, k
        same = np.array_equal(ibits(auto[k]), ibits(serial[k])) if auto[k].dtype == np.float32 else np.array_equal(auto[k], serial[k])
        assert same, (name, k)
    assert auto_stats == serial_stats, (name, auto_stats, serial_stats)
    # two launches per batch: the mirror rays had none of their own, and rode exactly once (the frames agree)
    assert auto_launches == want_launches and serial_launches < auto_launches, (name, serial_launches, auto_launches)
    if name in GOLDEN_ROWS:
        gold = np.load(os.path.join(GOLDEN, "scene_40x72_3spp_avg.npy")).reshape(40, 72, 3)[GOLDEN_ROWS[name]]
        assert np.array_equal(ibits(auto["avg"]), ibits(gold)), name
    if name == "every primary ray misses":
        assert not auto["avg"].any() and not auto["rgb"].any() and auto_stats[0] == 0
    elif name == "40x72@3":                                             # (an 8 x 8 frame of a few samples may well be black)
        assert auto["avg"].any() and auto_stats[0] > 0


def test_a_mirror_launch_of_its_own_is_one_launch_more(sqt, dev):
    """Option "mirror_ride" 0, the default: the automatic schedule as "overlap" 2 enqueues it.  The same frame, one trace launch more."""
    import torch
    call = frame_call(40, 72, 3)
    ride, ride_stats, ride_launches = run(sqt, torch, dev, call, AUTO, {})
    own, own_stats, own_launches = run(sqt, torch, dev, call, {"auto_overlap": 1, "auto_overlap_slots": 1}, {})
    assert own_launches == ride_launches + 1 == 7
    assert np.array_equal(ibits(own["avg"]), ibits(ride["avg"])) and np.array_equal(own["rgb"], ride["rgb"])
    assert own_stats[1:] == ride_stats[1:]


def test_small_frames_keep_the_serial_schedule_by_default(sqt, dev):
    """Under the library's own threshold a 64 x 64 frame at 4 samples is two trace launches, as it always was."""
    import torch
    out, _, launches = run(sqt, torch, dev, frame_call(64, 64, 4), {}, {})
    assert launches == 2
    assert np.array_equal(ibits(out["avg"]), ibits(np.load(os.path.join(GOLDEN, "scene_64x64_4spp_avg.npy")).reshape(64, 64, 3)))


def test_automatic_schedule_on_a_gated_side_stream(sqt, O, product_scene, oracle_scene):
    """The rig of tests/test_gpu_streams.py: the 64 x 64 @ 4 and 40 x 72 @ 3 frames of its `frames` job under the automatic schedule,
    on a non-blocking stream behind pending work, with a consumer behind them; the first frame is the committed golden one.
    (The rig takes three streams of torch's pool, which hands them out in turn over a few hardware queues: taken in front of
    tests/test_gpu_streams.py they decide which of that module's streams shares the null stream's queue, and its control then fails.
    This module sorts behind it.)"""
    import torch
    env = SH.Env(sqt, torch, O, product_scene[0], oracle_scene[0])
    try:
        env.set_options(env.ds)
        RO.set_options(env.ds, AUTO)
        env.ds.reset_timing()
        env.ds.enable_timing(True)
        env.ds.render_rows(env.new_cam(), 4, 64, 64)
        torch.cuda.synchronize()
        launches = env.ds.kernel_timing()[1]
        env.ds.enable_timing(False)
        env.ds.reset_timing()
        assert launches == 4                                            # the schedule under test: two pipelines of one batch each
        want = SH.drive(env, SH.job_frames(env, env.ds), env.side, "frames-auto_overlap")
        assert "sq_render_rows_device" in env.L.names
        SH.check_outside(env, "frames", want)
    finally:
        torch.cuda.synchronize()
        RO.set_options(env.ds, {"auto_overlap": 1, "auto_overlap_slots": 1 << 26, "mirror_ride": 0})
        env.close()
