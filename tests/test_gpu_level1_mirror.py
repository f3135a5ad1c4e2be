"""Condition (5) of level-1 culling on the GPU: every frame and query is bit-equal to the oracle with option "level1_cull" at 1 and
at 0; sq_get_stats slot 28 counts the rays conditions (1)-(3) drop, slot 29 those only condition (4) drops and slot 30 those only
condition (5) drops, each exactly what the restatements predict (tests/level1_restatement.py, tests/level1_stretch_restatement.py,
tests/level1_mirror_restatement.py), and all three stay 0 with the option off."""
import os

import numpy as np
import pytest

import level1_restatement as R
import level1_mirror_restatement as M5
import level1_stretch_restatement as S
from bitcmp import bits
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
CULLED, STRETCH, MIRROR = 28, 29, 30                                               # sq_get_stats slots
W, H, SPP = 40, 72, 3
CAM2 = b"0.5 6.5 0.9\n1.5707963267948966 0 -0.2\n"


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def scene(sqt, product_scene):
    bih, cam, _ = product_scene
    return sqt.DeviceScene(bih, 0), cam, R.tables(sqt, bih)[0], S.cover(sqt, bih), M5.mirror(sqt, bih)


@pytest.fixture(scope="module")
def predicted(scene, oracle_scene, sqt):
    """(first-bounce rays, culled by (1)-(3), by (4) alone, by (5) alone) of the 40 x 72 @ 3 frame, computed once."""
    _, _, T, V, M = scene
    ob, cam_o, _ = oracle_scene
    return M5.frame_prediction(sqt, T, V, M, ob, ob.flatten(), cam_o, SPP, W, H)


def counts(ds):
    st = ds.stats(reset=True)
    return int(st[CULLED]), int(st[STRETCH]), int(st[MIRROR])


@pytest.mark.parametrize("overlap", [0, 2])
def test_scene_obj_frame_and_the_three_predicted_counts(scene, predicted, torch, overlap):
    ds, cam, _, _, _ = scene
    fb, old, new, new5 = predicted
    want = np.load(os.path.join(GOLDEN, "scene_40x72_3spp_avg.npy"))
    ds.set_option("overlap", overlap)
    try:
        for on in (1, 0):
            ds.set_option("level1_cull", on)
            ds.stats(reset=True)
            avg, _ = ds.render_rows(cam, SPP, W, H)
            torch.cuda.synchronize()
            got = counts(ds)
            assert np.array_equal(bits(avg.cpu().numpy()), bits(want)), (on, overlap)
            assert ds.last_plan()["level1_cull"] == on
            print(f"{W}x{H} @ {SPP} overlap {overlap} level1_cull {on}: slots 28, 29, 30 = {got} of {len(old)} first-bounce rays; predicted {int(old.sum())}, {int(new.sum())}, {int(new5.sum())}")
            assert got == ((int(old.sum()), int(new.sum()), int(new5.sum())) if on else (0, 0, 0))
        assert 100 * int(new5.sum()) >= 8 * len(new5)                    # not vacuous (tests/test_level1_mirror.py): 8 % of the rays 1
    finally:
        ds.set_option("overlap", 0)
        ds.set_option("level1_cull", 1)


@pytest.mark.parametrize("make", [M5.axis_soup, M5.tilted_soup], ids=["axis_aligned_two_values", "tilted_plane"])
def test_soups_with_mirrors(sqt, O, torch, make):
    w = h = 16
    (tris, mats, ot), cam_txt = make()
    bih = sqt.BIH(sqt.Mesh.from_arrays(tris, mats))
    T, s = R.tables(sqt, bih)
    V, M = S.cover(sqt, bih), M5.mirror(sqt, bih)
    assert s["level1_on"] == 1 and V is not None and M["n_panels"] > 0
    cam_p, cam_o = sqt.camera_from_text(cam_txt), O.camera_from_text(cam_txt)
    ob = O.BIH(ot)
    want, _, _ = ob.render(cam_o, SPP, w, h, threads=min(os.cpu_count() or 1, 8))
    fb, old, new, new5 = M5.frame_prediction(sqt, T, V, M, ob, ob.flatten(), cam_o, SPP, w, h)
    assert new5.sum() > 0
    ds = sqt.DeviceScene(bih, 0)
    for on in (1, 0):
        ds.set_option("level1_cull", on)
        ds.stats(reset=True)
        avg, _ = ds.render_rows(cam_p, SPP, w, h)
        torch.cuda.synchronize()
        got = counts(ds)
        assert np.array_equal(bits(avg.cpu().numpy()), bits(want)), on
        print(f"{make.__name__} level1_cull {on}: slots 28, 29, 30 = {got} of {len(old)} first-bounce rays; predicted {int(old.sum())}, {int(new.sum())}, {int(new5.sum())}")
        assert got == ((int(old.sum()), int(new.sum()), int(new5.sum())) if on else (0, 0, 0))
    ds.close()


def test_views_masks_ranges_and_queries(scene, predicted, torch, oracle_scene, O, sqt):
    """The other ray sources and instantiations of sq_gen_bounce1: a two-view call, a range call split at an odd k, a masked call and a
    raytrace query under the frame's seeds -- each against the oracle's frame and the restatements' counts, with the option at 1 and at 0."""
    ds, cam, T, V, M = scene
    ob, cam_o, _ = oracle_scene
    fb, old, new, new5 = predicted
    want = np.load(os.path.join(GOLDEN, "scene_40x72_3spp_avg.npy"))
    cam2, cam2_o = sqt.camera_from_text(CAM2), O.camera_from_text(CAM2)
    want2, _, _ = ob.render(cam2_o, SPP, W, H, threads=min(os.cpu_count() or 1, 8))
    _, old2, new2, new52 = M5.frame_prediction(sqt, T, V, M, ob, ob.flatten(), cam2_o, SPP, W, H)
    dev = torch.device("cuda", 0)
    mask = torch.zeros((W, H), dtype=torch.uint8, device=dev)
    mask[::3, 1::2] = 1
    live = mask.cpu().numpy().astype(bool)
    in_mask = live[fb["y"], fb["x"]]
    whole = (int(old.sum()), int(new.sum()), int(new5.sum()))
    expect = {"views": (whole[0] + int(old2.sum()), whole[1] + int(new2.sum()), whole[2] + int(new52.sum())), "range": whole, "query": whole,
              "mask": (int((old & in_mask).sum()), int((new & in_mask).sum()), int((new5 & in_mask).sum()))}
    try:
        for on in (1, 0):
            got = {}
            ds.set_option("level1_cull", on)
            ds.stats(reset=True)
            avg, _ = ds.render_views([cam, cam2], SPP, W, H)
            assert np.array_equal(bits(avg[0].cpu().numpy()), bits(want)) and np.array_equal(bits(avg[1].cpu().numpy()), bits(want2)), on
            got["views"] = counts(ds)

            sums = torch.zeros((W, H, 3), dtype=torch.float32, device=dev)
            ds.render_rows_range(cam, SPP, W, H, 0, 1, sums)
            avg, _ = ds.render_rows_range(cam, SPP, W, H, 1, SPP, sums)
            assert np.array_equal(bits(avg.cpu().numpy()), bits(want)), on
            got["range"] = counts(ds)

            sums = torch.zeros((W, H, 3), dtype=torch.float32, device=dev)
            avg, _ = ds.render_rows_masked(cam, SPP, W, H, 0, SPP, sums, mask=mask)
            out = avg.cpu().numpy()
            assert np.array_equal(bits(out[live]), bits(want[live])) and not out[~live].any(), on
            got["mask"] = counts(ds)

            o, d = ds.camera_rays(cam, W, H)
            rad = ds.raytrace(o, d, seeds=sqt.device.frame_seeds(SPP, W, H, device=dev), samples=SPP)
            assert np.array_equal(bits(rad.avg.cpu().numpy()), bits(want)), on
            got["query"] = counts(ds)
            print(f"level1_cull {on}: slots 28, 29, 30 = {got}; predicted {expect}")
            assert got == (expect if on else dict.fromkeys(expect, (0, 0, 0)))
    finally:
        ds.set_option("level1_cull", 1)
    assert all(v[2] > 0 for v in expect.values()), expect
