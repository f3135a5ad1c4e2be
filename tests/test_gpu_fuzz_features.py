"""A slice of tests/fuzz_features.py: seeds 1000 .. 1399 -- the scenes and cameras of the frame campaign's own slice
(tests/test_gpu_parity.py) -- through caller-given depth, caller-given lights in every cast form, masked and multi-view calls and
the three ray queries, each against the oracle or its pinned restatement (tests/test_fuzz_features.py), bit for bit.  And the same
on the one shipped scene whose tree needs 4-byte stack words."""
import os
import sys

import numpy as np
import pytest

import depth_restatement as DR
import fuzz_features as FF
from conftest import ROOT
from lights_restatement import Restatement, avg_of, fold_cast
from ray_oracle import family_free

pytestmark = pytest.mark.gpu
f32 = np.float32
BLOCK = 25
# tools/gen_scenes.py's materials with light everywhere (as scenes.BRIGHT_SQ): a path's radiance tells which surfaces it met
BRIGHT_BLOB_SQ = (b"newmtl Diffuse\nreflective 0 0.700000 0.600000 0.500000\nemissive 0.25 0.9 0.5 0.2\n\n"
                  b"newmtl Glossy\nreflective 0.2 0.500000 0.300000 0.200000\nemissive 0.125 0.2 0.9 0.4\n\n"
                  b"newmtl Mirror\nreflective 1 0.900000 0.800000 0.700000\nemissive 0.5 0.3 0.6 0.9\n\n"
                  b"newmtl Light\nreflective 0 0 0 0\nemissive 60 1 1 1\n")
BLOCKS = [range(first, first + BLOCK) for first in range(1000, 1400, BLOCK)]


@pytest.mark.parametrize("seeds", BLOCKS, ids=[f"{b[0]}-{b[-1]}" for b in BLOCKS])
def test_a_block_of_seeds_equals_the_oracle_and_its_restatements(sqt, seeds):
    failures = [(seed, msg) for seed in seeds for msg in FF.run_case(seed)]
    assert not failures, failures


# Seeds the campaign found (python tests/fuzz_features.py 240 50000000).  All three: closed rooms whose materials pass the packer's
# nonneg_materials bound -- one product, the reference's depth -- while two or more nested products overflow: under depth 4 and 5 the
# radiance below an absorbing surface is inf, 0 * inf is NaN in the reference, and the wavefront form's shortcut wrote +0 there.
REGRESSIONS = (50002805, 50004673, 50005366)


@pytest.mark.parametrize("seed", REGRESSIONS)
def test_a_seed_the_campaign_found(sqt, seed):
    assert FF.run_case(seed) == []


def test_the_blob_with_4_byte_stack_words_at_depth_5_and_under_three_lights(sqt, O):
    """500 rays (the camera's and free ones, with small, huge and negative seeds) at depth 5, and a 12 x 16 cast frame under three
    lights, in the per-lane form, the default form and the streaming form, against the two restatements."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_scenes as G
    obj, _, camt = (t.encode() if isinstance(t, str) else t for t in G.blob_scene(6))
    sq = BRIGHT_BLOB_SQ
    bih = sqt.BIH(sqt.Mesh.from_text(obj, sq))
    ob = O.BIH(O.tris_from_text(obj, sq))
    flat = ob.flatten()
    cam, ocam = sqt.camera_from_text(camt), O.camera_from_text(camt)
    w, h, spp = 12, 16, 2
    cam_rays = [O.make_ray(w, h, y, x, ocam) for y in range(w) for x in range(h)]
    rng = np.random.default_rng(3)
    fo, fd = family_free(rng, bih.bounds, 2000)
    fd = FF.positive_zeros(fd)
    keep = DR.first_hitting(ob, fo, fd, 500 - w * h)
    fo, fd = fo[keep], fd[keep]
    o = np.ascontiguousarray(np.concatenate([np.array([r[0] for r in cam_rays], f32), fo]))
    d = FF.positive_zeros(np.concatenate([np.array([r[1] for r in cam_rays], f32), fd]))
    third = np.arange(500) % 3
    s = np.where(third == 0, rng.integers(0, 1 << 20, 500), np.where(third == 1, rng.integers(1 << 40, 1 << 60, 500), -rng.integers(1, 1 << 60, 500)))
    trails = DR.paths(ob, flat, o, d, s, depth=5)
    want_rays = FF.from_zero(DR.radiances(trails, 5))
    assert (want_rays != 0).any(-1).mean() > 0.5
    assert (FF.canon(want_rays) != FF.canon(FF.from_zero(DR.radiances(trails, 3)))).any(-1).mean() > 0.25      # depth 5 is not depth 3
    lights = [((0, 3, -1), (2, 1, 0.5)), ((1.5, -2, 0.5), (0.25, 2, 1)), ((-1, 1, 1.5), (3, 0.75, 0.5))]
    T, lit = Restatement(O, ob).radiance("frame", cam_rays, lights)
    assert ((lit == 1).any(0) & (lit == 0).any(0)).all(), "every light lights and shadows a hit pixel"
    want_avg = avg_of(fold_cast(T, 0, spp), spp).reshape(w, h, 3)
    want_rgb = FF.tonemaps(want_avg)
    ds = sqt.DeviceScene(bih, 0)
    try:
        ds.set_depth(5)
        ds.set_lights(lights)
        for opts in ({"variant": 1}, {}, {"resident": 0}):
            for k, v in {"variant": 2, "resident": 1, "cast_wavefront": 1, **opts}.items():
                ds.set_option(k, v)
            got = ds.raytrace(o, d, seeds=s).sum
            torch.cuda.synchronize()
            assert ds.last_plan()["stack_word_bytes"] == 4 and ds.last_plan()["launched"] == 1, (opts, ds.last_plan())
            assert FF.same(got.cpu().numpy(), want_rays), (opts, "rays")
            avg, rgb = ds.render_rows(cam, spp, w, h, cast=True)
            torch.cuda.synchronize()
            assert FF.same(avg.cpu().numpy(), want_avg) and np.array_equal(rgb.cpu().numpy(), want_rgb), (opts, "cast frame")
    finally:
        ds.close()
