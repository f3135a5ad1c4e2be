"""sq_shade1 with many samples in a lane.  The kernel's thread walks the samples blockIdx.y + j * gridDim.y of its pixel, requesting
slots one and two samples ahead; a frame of test size gets gridDim.y = min(samples of the batch, 64), so a lane holds samples / 64 of
them, and the other GPU tests stay at a handful of samples per pixel.  The frames here put 1, 2 or 3 (the depth of the prefetch), 31
or 32, 32, 32 or 33 and 67 or 68 samples into a lane: 64, 130, 2047, 2048, 2049 and 4300 spp.  The counts around W = 32 were chosen
for a walk in windows of 32 samples -- a bit mask of a window's unfinished slots, taken lowest bit first -- which passed these tests
and was not kept: it measured slower (profiles/r10a_per_sample_divergence.txt).  Whatever loop the kernel has must pass
them.  Every frame is data/scene.obj under the sample camera, small enough that wall, monkey (every sample mirrored) and lamp
(absorbing) pixels share a wave, and bit-equal to the oracle's; so are the same frames through the range, masked, multi-view
(sq_shade1<1>) and ray-query (sq_shade1<2>) calls, the overlapped schedule and workspaces that force several batches.

Counters.  sq_get_stats slots 28-30 (written by sq_gen_bounce1) equal the numpy restatements' prediction on the 64 spp frame, where
Python can walk every sample, and on every other call they and slot 0 (the rays the trace launches took, which follow from the states
sq_shade1 leaves behind) equal those of the plain call of the same frame.  Slot 0 is not compared for range calls: each call traces
the pixels' mirror rays again."""
import os

import numpy as np
import pytest

import level1_mirror_restatement as M5
import level1_restatement as R
import level1_stretch_restatement as S
from bitcmp import bits

pytestmark = pytest.mark.gpu
WINDOW = 32
SLOTS = (0, 28, 29, 30)
FRAMES = {64: (12, 10), 130: (8, 9), 2047: (9, 9), 2048: (10, 9), 2049: (8, 9), 4300: (12, 10)}      # spp: (rows, columns); eight columns show no lamp
CAM2 = b"0.5 6.5 0.9\n1.5707963267948966 0 -0.2\n"
THREADS = min(os.cpu_count() or 1, 8)


def test_sample_counts_sit_on_the_window_edges():
    per_lane = {spp: {(spp - y + 63) // 64 for y in range(64)} for spp in FRAMES}
    assert per_lane == {64: {1}, 130: {2, 3}, 2047: {WINDOW - 1, WINDOW}, 2048: {WINDOW}, 2049: {WINDOW, WINDOW + 1}, 4300: {2 * WINDOW + 3, 2 * WINDOW + 4}}
    assert all(8 * 8 <= w * h <= 12 * 10 for w, h in FRAMES.values())


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def ds(sqt, product_scene):
    d = sqt.DeviceScene(product_scene[0], 0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def wanted(oracle_scene, O):
    """spp (and optionally a camera text) -> the oracle's frame, each rendered once."""
    ob, cam_o, _ = oracle_scene
    cache = {}

    def get(spp, cam_txt=None):
        if (spp, cam_txt) not in cache:
            w, h = FRAMES[spp]
            cache[spp, cam_txt] = ob.render(O.camera_from_text(cam_txt) if cam_txt else cam_o, spp, w, h, threads=THREADS, want_rgb=False)[0]
        return cache[spp, cam_txt]
    return get


def counters(ds):
    st = ds.stats(reset=True)
    return tuple(int(st[i]) for i in SLOTS)


@pytest.fixture(scope="module")
def plain(ds, product_scene, sqt, torch, wanted):
    """spp (and optionally a camera text) -> the counters of the plain render_rows call of that frame, which is checked against the oracle."""
    cache = {}

    def get(spp, cam_txt=None):
        if (spp, cam_txt) not in cache:
            w, h = FRAMES[spp]
            ds.stats(reset=True)
            avg, _ = ds.render_rows(sqt.camera_from_text(cam_txt) if cam_txt else product_scene[1], spp, w, h)
            torch.cuda.synchronize()
            cache[spp, cam_txt] = counters(ds)
            assert np.array_equal(bits(avg.cpu().numpy()), bits(wanted(spp, cam_txt))), (spp, cam_txt)
        return cache[spp, cam_txt]
    return get


def test_every_frame_holds_wall_monkey_and_lamp_pixels(oracle_scene, O):
    ob, cam_o, _ = oracle_scene
    flat = ob.flatten()
    for w, h in set(FRAMES.values()):
        kinds = set()
        for y in range(w):
            for x in range(h):
                hit = ob.intersect(*O.make_ray(w, h, y, x, cam_o))
                if hit.hit:
                    t = flat[hit.tri]
                    kinds.add("lamp" if not t["surf"].any() else "monkey" if t["reflective"] >= 1 else "wall")
        assert kinds == {"lamp", "monkey", "wall"}, (w, h, kinds)


@pytest.mark.parametrize("overlap", [0, 2])
@pytest.mark.parametrize("spp", sorted(FRAMES))
def test_frames_at_the_window_edges(ds, product_scene, torch, wanted, plain, spp, overlap):
    w, h = FRAMES[spp]
    base = plain(spp)
    ds.set_option("overlap", overlap)
    try:
        ds.stats(reset=True)
        avg, _ = ds.render_rows(product_scene[1], spp, w, h)
        torch.cuda.synchronize()
        got = counters(ds)
    finally:
        ds.set_option("overlap", 0)
    print(f"{w}x{h} @ {spp} overlap {overlap}: slots 0, 28, 29, 30 = {got}; plain call {base}")
    assert np.array_equal(bits(avg.cpu().numpy()), bits(wanted(spp)))
    assert got == base


def test_level1_counters_are_the_restatements_prediction(sqt, product_scene, oracle_scene, plain):
    spp = 64
    w, h = FRAMES[spp]
    bih = product_scene[0]
    ob, cam_o, _ = oracle_scene
    _, old, new, new5 = M5.frame_prediction(sqt, R.tables(sqt, bih)[0], S.cover(sqt, bih), M5.mirror(sqt, bih), ob, ob.flatten(), cam_o, spp, w, h)
    got = plain(spp)
    print(f"{w}x{h} @ {spp}: slots 28, 29, 30 = {got[1:]} of {len(old)} first-bounce rays; predicted {int(old.sum())}, {int(new.sum())}, {int(new5.sum())}")
    assert got[1:] == (int(old.sum()), int(new.sum()), int(new5.sum()))
    assert old.sum() > 0 and new.sum() > 0 and new5.sum() > 0


@pytest.mark.parametrize("spp,cuts", [(2049, (0, 33, 2049)), (4300, (0, 2111, 2112, 4300))], ids=["2049", "4300"])
def test_ranges_that_cut_a_window(ds, product_scene, torch, wanted, plain, spp, cuts):
    """Each call's samples start anew at the lane's bit 0: 33 samples (1 or no sample in a lane), 2016 (31 or 32), 2111 (32 or 33), 1, 2188 (34 or 35)."""
    w, h = FRAMES[spp]
    base = plain(spp)
    sums = torch.zeros((w, h, 3), dtype=torch.float32, device=torch.device("cuda", 0))
    ds.stats(reset=True)
    for k0, k1 in zip(cuts, cuts[1:]):
        avg, _ = ds.render_rows_range(product_scene[1], spp, w, h, k0, k1, sums)
    torch.cuda.synchronize()
    got = counters(ds)
    print(f"{w}x{h} @ {spp} in ranges {cuts}: slots 0, 28, 29, 30 = {got}; plain call {base}")
    assert np.array_equal(bits(avg.cpu().numpy()), bits(wanted(spp)))
    assert got[1:] == base[1:]


def test_a_mask_and_its_complement(ds, product_scene, torch, wanted, plain):
    spp = 2049
    w, h = FRAMES[spp]
    base, want = plain(spp), wanted(spp)
    dev = torch.device("cuda", 0)
    mask = torch.zeros((w, h), dtype=torch.uint8, device=dev)
    mask[::3, 1::2] = 1
    mask[1, :] = 1
    total = np.zeros(len(SLOTS), np.int64)
    for m in (mask, 1 - mask):
        live = m.cpu().numpy().astype(bool)
        sums = torch.zeros((w, h, 3), dtype=torch.float32, device=dev)
        ds.stats(reset=True)
        avg, _ = ds.render_rows_masked(product_scene[1], spp, w, h, 0, spp, sums, mask=m)
        out = avg.cpu().numpy()
        total += counters(ds)
        assert np.array_equal(bits(out[live]), bits(want[live])) and not out[~live].any()
    total = tuple(int(v) for v in total)
    print(f"{w}x{h} @ {spp}, a mask and its complement: slots 0, 28, 29, 30 sum to {total}; plain call {base}")
    assert total == base


def test_two_views(ds, sqt, product_scene, torch, wanted, plain):
    spp = 2049
    w, h = FRAMES[spp]
    base = tuple(a + b for a, b in zip(plain(spp), plain(spp, CAM2)))
    ds.stats(reset=True)
    avg, _ = ds.render_views([product_scene[1], sqt.camera_from_text(CAM2)], spp, w, h)
    torch.cuda.synchronize()
    got = counters(ds)
    print(f"{w}x{h} @ {spp}, two views: slots 0, 28, 29, 30 = {got}; the two plain calls {base}")
    assert np.array_equal(bits(avg[0].cpu().numpy()), bits(wanted(spp))) and np.array_equal(bits(avg[1].cpu().numpy()), bits(wanted(spp, CAM2)))
    assert got == base


def test_ray_query_of_the_camera_rays(ds, sqt, product_scene, torch, wanted, plain):
    spp = 2049
    w, h = FRAMES[spp]
    base = plain(spp)
    o, d = ds.camera_rays(product_scene[1], w, h)
    ds.stats(reset=True)
    rad = ds.raytrace(o, d, seeds=sqt.device.frame_seeds(spp, w, h, device=torch.device("cuda", 0)), samples=spp)
    torch.cuda.synchronize()
    got = counters(ds)
    print(f"{w}x{h} @ {spp}, raytrace of the camera rays: slots 0, 28, 29, 30 = {got}; plain call {base}")
    assert np.array_equal(bits(rad.avg.cpu().numpy()), bits(wanted(spp)))
    assert got == base


@pytest.mark.parametrize("per_pixel", [1500, 2200])
def test_several_batches(ds, product_scene, torch, wanted, plain, per_pixel):
    """4300 samples in a workspace of 1500 slots per pixel: batches of 1434, 1434 and 1432 (22 or 23 samples in a lane); of 2200: 2150 and 2150 (33 or 34)."""
    spp = 4300
    w, h = FRAMES[spp]
    base = plain(spp)
    ds.set_option("slots", w * h * per_pixel)
    try:
        ds.stats(reset=True)
        avg, _ = ds.render_rows(product_scene[1], spp, w, h)
        torch.cuda.synchronize()
        got = counters(ds)
    finally:
        ds.set_option("slots", 512 << 20)
    print(f"{w}x{h} @ {spp}, {per_pixel} slots per pixel: slots 0, 28, 29, 30 = {got}; plain call {base}")
    assert np.array_equal(bits(avg.cpu().numpy()), bits(wanted(spp)))
    assert got == base
