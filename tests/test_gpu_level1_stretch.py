"""Condition (4) of level-1 culling on the GPU: every frame and query is bit-equal to the oracle with option "level1_cull" at 1 and
at 0; sq_get_stats slot 28 counts the rays conditions (1)-(3) drop and slot 29 those only condition (4) drops, each exactly what the
restatements predict (tests/level1_restatement.py, tests/level1_stretch_restatement.py), and both stay 0 with the option off."""
import os

import numpy as np
import pytest

import level1_restatement as R
import level1_stretch_restatement as S
from bitcmp import bits
from conftest import GOLDEN
from level1_restatement import soup

pytestmark = pytest.mark.gpu
CULLED, STRETCH = 28, 29                                                # sq_get_stats slots
W, H, SPP = 40, 72, 3
CAM2 = b"0.5 6.5 0.9\n1.5707963267948966 0 -0.2\n"


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def scene(sqt, product_scene):
    bih, cam, _ = product_scene
    return sqt.DeviceScene(bih, 0), cam, R.tables(sqt, bih)[0], S.cover(sqt, bih)


@pytest.fixture(scope="module")
def predicted(scene, oracle_scene, sqt):
    """(first-bounce rays, culled by (1)-(3), culled by (4) alone) of the 40 x 72 @ 3 frame, computed once."""
    _, _, T, V = scene
    ob, cam_o, _ = oracle_scene
    return S.frame_prediction(sqt, T, V, ob, ob.flatten(), cam_o, SPP, W, H)


def counts(ds):
    st = ds.stats(reset=True)
    return int(st[CULLED]), int(st[STRETCH])


@pytest.mark.parametrize("overlap", [0, 2])
def test_scene_obj_frame_and_both_predicted_counts(scene, predicted, torch, overlap):
    ds, cam, _, _ = scene
    fb, old, new = predicted
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
            print(f"{W}x{H} @ {SPP} overlap {overlap} level1_cull {on}: slots 28, 29 = {got} of {len(old)} first-bounce rays; predicted {int(old.sum())}, {int(new.sum())}")
            assert got == ((int(old.sum()), int(new.sum())) if on else (0, 0))
        assert 20 * int(new.sum()) >= len(new)                           # not vacuous (tests/test_level1_stretch.py): one ray 1 in twenty
    finally:
        ds.set_option("overlap", 0)
        ds.set_option("level1_cull", 1)


# (seed, emitters, camera, soup arguments) as tests/test_gpu_level1_cull.py draws them: one large emitter seen from outside, and twelve
# clustered ones seen from inside their box
SOUPS = [(21, 1, b"-6 0.1 0.2\n0 0 0\n", {"zoned": (1.2, -1.2, -1.2), "emitter_size": 0.8}),
         (23, 12, None, {"zoned": (1.2, -1.2, -1.2), "cluster": (-1.0, 1.0, 1.0)})]


@pytest.mark.parametrize("seed,n_emit,cam_txt,kw", SOUPS)
def test_random_soups(sqt, O, torch, seed, n_emit, cam_txt, kw):
    w = h = 16
    tris, mats, ot = soup(seed, n_emit, **kw)
    bih = sqt.BIH(sqt.Mesh.from_arrays(tris, mats))
    T, s = R.tables(sqt, bih)
    V = S.cover(sqt, bih)
    assert s["level1_on"] == 1 and V is not None
    if cam_txt is None:                                                  # inside the emitters' box
        c = (T["em_lo"] + T["em_hi"]) / 2
        cam_txt = f"{c[0]} {c[1]} {c[2]}\n0.3 0.2 0.1\n".encode()
    cam_p, cam_o = sqt.camera_from_text(cam_txt), O.camera_from_text(cam_txt)
    ob = O.BIH(ot)
    want, _, _ = ob.render(cam_o, SPP, w, h, threads=min(os.cpu_count() or 1, 8))
    fb, old, new = S.frame_prediction(sqt, T, V, ob, ob.flatten(), cam_o, SPP, w, h)
    ds = sqt.DeviceScene(bih, 0)
    for on in (1, 0):
        ds.set_option("level1_cull", on)
        ds.stats(reset=True)
        avg, _ = ds.render_rows(cam_p, SPP, w, h)
        torch.cuda.synchronize()
        got = counts(ds)
        assert np.array_equal(bits(avg.cpu().numpy()), bits(want)), on
        print(f"soup {seed} ({n_emit} emitters) level1_cull {on}: slots 28, 29 = {got} of {len(old)} first-bounce rays; predicted {int(old.sum())}, {int(new.sum())}")
        assert got == ((int(old.sum()), int(new.sum())) if on else (0, 0))
    ds.close()


def test_views_masks_ranges_and_queries(scene, predicted, torch, oracle_scene, O, sqt):
    """The other ray sources and instantiations of sq_gen_bounce1: a two-view call, a range call split at an odd k, a masked call and a
    raytrace query under the frame's seeds -- each against the oracle's frame and the restatements' counts, with the option at 1 and at 0."""
    ds, cam, T, V = scene
    ob, cam_o, _ = oracle_scene
    fb, old, new = predicted
    want = np.load(os.path.join(GOLDEN, "scene_40x72_3spp_avg.npy"))
    cam2, cam2_o = sqt.camera_from_text(CAM2), O.camera_from_text(CAM2)
    want2, _, _ = ob.render(cam2_o, SPP, W, H, threads=min(os.cpu_count() or 1, 8))
    _, old2, new2 = S.frame_prediction(sqt, T, V, ob, ob.flatten(), cam2_o, SPP, W, H)
    dev = torch.device("cuda", 0)
    mask = torch.zeros((W, H), dtype=torch.uint8, device=dev)
    mask[::3, 1::2] = 1
    live = mask.cpu().numpy().astype(bool)
    in_mask = live[fb["y"], fb["x"]]
    whole = (int(old.sum()), int(new.sum()))
    expect = {"views": (whole[0] + int(old2.sum()), whole[1] + int(new2.sum())), "range": whole, "query": whole,
              "mask": (int((old & in_mask).sum()), int((new & in_mask).sum()))}
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
            print(f"level1_cull {on}: slots 28, 29 = {got}; predicted {expect}")
            assert got == (expect if on else dict.fromkeys(expect, (0, 0)))
    finally:
        ds.set_option("level1_cull", 1)
    assert all(v[1] > 0 for v in expect.values()), expect
