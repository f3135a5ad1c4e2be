"""The inputs of tests/test_gpu_fuzz_features.py, judged without a GPU: on every seed of the slice the two restatements the GPU tests
compare with are the C oracle's own frames where the oracle can say (depth 3, the reference's light), bit for bit; and the slice
holds enough of every case the newer kernels branch on, counted from the restatements and the packer alone."""
import numpy as np
import pytest

import fuzz_features as FF
import level1_restatement
from scenes import pack

SEEDS = range(1000, 1400)
canon = FF.canon


class Row:
    pass


@pytest.fixture(scope="module")
def table(sqt, O):
    """One Row per seed: the two pins and the facts the coverage conditions count."""
    out = []
    for seed in SEEDS:
        c = FF.case(seed)
        r = Row()
        r.seed = seed
        # the pins
        _, _, avg3, rgb3 = FF.deep_frame(c, 3)
        want, want8 = FF.oracle_frame(c, cast=False)
        r.depth_pin = np.array_equal(canon(avg3), canon(want)) and np.array_equal(rgb3, want8)
        cast, cast8, _, _ = FF.cast_frame(c, [sqt.REFERENCE_LIGHT])
        want, want8 = FF.oracle_frame(c, cast=True)
        r.lights_pin = np.array_equal(canon(cast), canon(want)) and np.array_equal(cast8, want8)
        # the ray batch: the restatement at depth 3 is the oracle's raytrace of every ray, and with the reference's light its raycast
        ro, rd, rs = FF.radiance_rays(c)
        r.rays_pin = np.array_equal(canon(DR_radiances(c, 3)), canon(FF.oracle_raytrace(O, c.ob, ro, rd, rs)))
        T, _ = FF.restatement(c).radiance("batch", list(zip(ro, rd)), [sqt.REFERENCE_LIGHT])
        r.raycast_pin = np.array_equal(canon(FF.avg_of(FF.fold_cast(T, 0, 1), 1)), canon(FF.oracle_raycast(O, c.ob, ro, rd)))
        # coverage, from the restatements and the packer
        _, _, avgD, _ = FF.deep_frame(c, c.depth)
        r.depth_changes = not np.array_equal(canon(avgD), canon(avg3))
        r.alive_at_3 = c.depth >= 4 and any(len(t) > 3 and t[3] is not None for trails in FF.frame_paths(c) for t in trails)
        r.nan_frame = bool(np.isnan(avgD).any())
        arrays, scalars = pack(sqt, FF.product_bih(c))
        r.long_leaf = FF.product_bih(c).longest_leaf > 31
        assert r.long_leaf == (scalars["packed_leaves"] == 0)
        r.emitters = len(arrays["emitters"]) // 4
        r.nonneg = scalars["nonneg_materials"]
        r.tris = len(c.v)
        _, _, _, lit = FF.cast_frame(c, FF.light_pairs(c.lights))
        r.lights_seen = bool(((lit == 1).any(0) & (lit == 0).any(0)).all())
        r.height = FF.product_bih(c).height
        # the plan turns level-1 culling on for the three-level pipeline alone: with deep = 0, the depth-3 queries of the case run it
        r.level1_knob = c.knobs["level1_cull"] if level1_restatement.tables(sqt, FF.product_bih(c))[1]["level1_on"] and not c.deep else None
        out.append(r)
    return out


def DR_radiances(c, depth):
    return FF.DR.radiances(FF.ray_paths(c), depth)


def test_the_depth_restatement_at_depth_3_is_the_oracles_frame_on_every_seed(table):
    assert [r.seed for r in table if not r.depth_pin] == []


def test_the_lights_restatement_with_the_reference_light_is_the_oracles_cast_frame_on_every_seed(table):
    assert [r.seed for r in table if not r.lights_pin] == []


def test_the_restatements_are_the_oracles_raytrace_and_raycast_of_every_ray_of_the_batches(table):
    assert [r.seed for r in table if not r.rays_pin] == [] and [r.seed for r in table if not r.raycast_pin] == []


COVERAGE = (
    ("the drawn depth changes the frame's bits against depth 3", lambda r: r.depth_changes, len(SEEDS) // 4),
    ("a sample is alive at level 3 or deeper", lambda r: r.alive_at_3, 40),
    ("NaN in the expected deep frame", lambda r: r.nan_frame, 15),
    ("a leaf longer than 31", lambda r: r.long_leaf, 40),
    ("exactly 64 or 65 emitters", lambda r: r.emitters in (64, 65), 10),
    ("no emitter", lambda r: r.emitters == 0, 10),
    ("nonneg_materials off", lambda r: r.nonneg == 0, 40),
    ("at most 16 triangles", lambda r: r.tris <= 16, 20),
    ("every drawn light lights and shadows a hit pixel", lambda r: r.lights_seen, 50),
)


def test_level_1_culling_is_drawn_on_and_off_among_the_cases_whose_plan_turns_it_on(table):
    assert {r.level1_knob for r in table} >= {0, 1}, [r.level1_knob for r in table].count(None)


@pytest.mark.parametrize("what, fact, least", COVERAGE, ids=[c[0] for c in COVERAGE])
def test_the_slice_covers(table, what, fact, least):
    count = sum(1 for r in table if fact(r))
    print(f"seeds 1000..1399 where {what}: {count} (at least {least} asked); tallest tree {max(r.height for r in table)}")
    assert count >= least, f"{what}: {count} seeds, {least} asked"
