"""Level-1 culling on the GPU: every frame and query is bit-equal to the oracle with option "level1_cull" at 1 and at 0, and the
rays it drops are the ones tests/level1_restatement.py predicts (none with the option off)."""
import os

import numpy as np
import pytest

import level1_restatement as R
from bitcmp import bits
from conftest import DATA, GOLDEN
from level1_restatement import soup

pytestmark = pytest.mark.gpu
CULLED = 28                                                             # sq_get_stats slot


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def scene(sqt, product_scene):
    bih, cam, _ = product_scene
    return sqt.DeviceScene(bih, 0), cam, R.tables(sqt, bih)[0]


def frame(ds, torch, cam, spp, w, h, on, **kw):
    """(avg, rgb8, rays culled, plan) of one render_rows call under level1_cull = on."""
    ds.set_option("level1_cull", on)
    ds.stats(reset=True)
    avg, rgb = ds.render_rows(cam, spp, w, h, **kw)
    torch.cuda.synchronize()
    return avg.cpu().numpy(), rgb.cpu().numpy(), ds.stats()[CULLED], ds.last_plan()


@pytest.mark.parametrize("w,h,spp,overlap", [(64, 64, 4, 0), (40, 72, 3, 0), (64, 64, 4, 1), (64, 64, 4, 2)])
def test_scene_obj_frames_and_the_predicted_count(scene, torch, oracle_scene, sqt, w, h, spp, overlap):
    ds, cam, T = scene
    ob, cam_o, _ = oracle_scene
    if (w, h, spp) == (64, 64, 4):
        want, want8 = np.load(os.path.join(GOLDEN, "scene_64x64_4spp_avg.npy")), np.load(os.path.join(GOLDEN, "scene_64x64_4spp_rgb8.npy"))
    else:
        want, want8, _ = ob.render(cam_o, spp, w, h, threads=min(os.cpu_count() or 1, 8))
        assert np.array_equal(bits(want), bits(np.load(os.path.join(GOLDEN, "scene_40x72_3spp_avg.npy"))))
    fb, predicted = R.frame_prediction(sqt, T, ob, ob.flatten(), cam_o, spp, w, h)
    ds.set_option("overlap", overlap)
    try:
        for on in (1, 0):
            avg, rgb, culled, plan = frame(ds, torch, cam, spp, w, h, on)
            assert np.array_equal(bits(avg), bits(want)) and np.array_equal(rgb, want8), (on, int((bits(avg) != bits(want)).any(-1).sum()))
            assert plan["level1_cull"] == on
            print(f"{w}x{h} @ {spp} overlap {overlap} level1_cull {on}: {culled} of {len(predicted)} first-bounce rays culled, predicted {int(predicted.sum())}")
            assert culled == (int(predicted.sum()) if on else 0)
            if on:
                assert 10 * culled >= len(predicted)                     # not vacuous: at least one first-bounce ray in ten
    finally:
        ds.set_option("overlap", 0)
        ds.set_option("level1_cull", 1)


# (seed, emitters, w, h, spp, camera, soup arguments): an emitter touching and grazing other geometry in every soup (soup());
# 1, 2, 12 and 65 emitters; reflective values on both sides of the class cuts (six values, four classes) and an always-mirror
# material; a camera inside the emitters' box
SOUPS = [(21, 1, 16, 16, 16, b"-6 0.1 0.2\n0 0 0\n", {"zoned": (1.2, -1.2, -1.2), "emitter_size": 0.8}),
         (22, 2, 24, 24, 8, b"-6 0.1 0.2\n0 0 0\n", {"zoned": (-1.2, -1.2, -1.2), "cluster": (1.2, 1.2, -1.2), "emitter_size": 0.6}),
         (23, 12, 48, 48, 4, None, {"zoned": (1.2, -1.2, -1.2), "cluster": (-1.0, 1.0, 1.0)}),
         (24, 65, 32, 32, 4, b"-6 0.1 0.2\n0 0 0\n", {"zoned": (1.2, -1.2, -1.2)}),
         (25, 2, 24, 24, 8, b"-6 0.1 0.2\n0 0 0\n", {"reflective": (0.0, 1.0), "zoned": (1.2, 1.2, 1.2), "cluster": (1.2, -1.2, 1.2), "emitter_size": 0.6})]


@pytest.mark.parametrize("seed,n_emit,w,h,spp,cam_txt,kw", SOUPS)
def test_random_soups(sqt, O, torch, seed, n_emit, w, h, spp, cam_txt, kw):
    tris, mats, ot = soup(seed, n_emit, **kw)
    bih = sqt.BIH(sqt.Mesh.from_arrays(tris, mats))
    T, s = R.tables(sqt, bih)
    if cam_txt is None:                                                  # inside the emitters' box
        c = (T["em_lo"] + T["em_hi"]) / 2
        cam_txt = f"{c[0]} {c[1]} {c[2]}\n0.3 0.2 0.1\n".encode()
    cam_p, cam_o = sqt.camera_from_text(cam_txt), O.camera_from_text(cam_txt)
    ob = O.BIH(ot)
    want, want8, _ = ob.render(cam_o, spp, w, h, threads=min(os.cpu_count() or 1, 8))
    fb, predicted = R.frame_prediction(sqt, T, ob, ob.flatten(), cam_o, spp, w, h)
    ds = sqt.DeviceScene(bih, 0)
    for on in (1, 0):
        avg, rgb, culled, plan = frame(ds, torch, cam_p, spp, w, h, on)
        assert np.array_equal(bits(avg), bits(want)) and np.array_equal(rgb, want8), (on, int((bits(avg) != bits(want)).any(-1).sum()))
        assert plan["level1_cull"] == (on if n_emit <= 64 else 0)
        print(f"soup {seed} ({n_emit} emitters) level1_cull {on}: {culled} of {len(predicted)} first-bounce rays culled, predicted {int(predicted.sum())}")
        assert culled == (int(predicted.sum()) if on else 0)
    assert s["level1_on"] == (n_emit <= 64) and (predicted.any() or n_emit > 12)
    ds.close()


def test_views_masks_ranges_and_queries(scene, torch, oracle_scene, O, sqt):
    """The other ray sources and instantiations of sq_gen_bounce1: a two-view call, a masked call, a range call split at an odd k
    and a raytrace query under the frame's seeds -- each against the oracle's frame, with the option at 1 and at 0."""
    ds, cam, T = scene
    ob, cam_o, _ = oracle_scene
    w, h, spp = 40, 72, 3
    want = np.load(os.path.join(GOLDEN, "scene_40x72_3spp_avg.npy"))
    cam2_txt = b"0.5 6.5 0.9\n1.5707963267948966 0 -0.2\n"
    cam2, cam2_o = sqt.camera_from_text(cam2_txt), O.camera_from_text(cam2_txt)
    want2, _, _ = ob.render(cam2_o, spp, w, h, threads=min(os.cpu_count() or 1, 8))
    dev = torch.device("cuda", 0)
    counts = {}
    try:
        for on in (1, 0):
            ds.set_option("level1_cull", on)
            ds.stats(reset=True)
            avg, _ = ds.render_views([cam, cam2], spp, w, h)
            assert np.array_equal(bits(avg[0].cpu().numpy()), bits(want)) and np.array_equal(bits(avg[1].cpu().numpy()), bits(want2)), on
            counts[on, "views"] = ds.stats(reset=True)[CULLED]

            sums = torch.zeros((w, h, 3), dtype=torch.float32, device=dev)
            ds.render_rows_range(cam, spp, w, h, 0, 1, sums)
            avg, _ = ds.render_rows_range(cam, spp, w, h, 1, spp, sums)
            assert np.array_equal(bits(avg.cpu().numpy()), bits(want)), on
            counts[on, "range"] = ds.stats(reset=True)[CULLED]

            mask = torch.zeros((w, h), dtype=torch.uint8, device=dev)
            mask[::3, 1::2] = 1
            sums = torch.zeros((w, h, 3), dtype=torch.float32, device=dev)
            avg, _ = ds.render_rows_masked(cam, spp, w, h, 0, spp, sums, mask=mask)
            live = mask.cpu().numpy().astype(bool)
            got = avg.cpu().numpy()
            assert np.array_equal(bits(got[live]), bits(want[live])) and not got[~live].any(), on
            counts[on, "mask"] = ds.stats(reset=True)[CULLED]

            o, d = ds.camera_rays(cam, w, h)
            rad = ds.raytrace(o, d, seeds=sqt.device.frame_seeds(spp, w, h, device=dev), samples=spp)
            assert np.array_equal(bits(rad.avg.cpu().numpy()), bits(want)), on
            counts[on, "query"] = ds.stats(reset=True)[CULLED]
    finally:
        ds.set_option("level1_cull", 1)
    print(counts)
    for what in ("views", "range", "mask", "query"):
        assert counts[0, what] == 0 and counts[1, what] > 0, (what, counts)
    assert counts[1, "range"] == counts[1, "query"] and counts[1, "views"] > counts[1, "range"] > counts[1, "mask"]
