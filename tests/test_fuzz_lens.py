"""The inputs of tests/test_gpu_fuzz_lens.py, judged without a GPU: on every seed of the slice the lens and shutter restatements are
the oracle's frame, each other, and depth_restatement where they meet off the room; the triangle tables the guides are compared with
are the product's own; and the slice holds enough of every case the lens, shutter and temporal kernels branch on, counted from the
restatements alone."""
import numpy as np
import pytest

import depth_restatement as DR
import fuzz_features as FF
import fuzz_lens as FL
import lens_restatement as LR
import shutter_restatement as SHR
import sky_restatement as SR
import temporal_restatement as TR
from bitcmp import same

SEEDS = FL.SLICE
f32 = np.float32


class Row:
    pass


def same_rays(a, b):
    return same(a[0], b[0]) and same(a[1], b[1]) and np.array_equal(a[2], b[2])


@pytest.fixture(scope="module")
def table(sqt, O):
    """One Row per seed: the pins and the facts the coverage conditions count."""
    out = []
    for seed in SEEDS:
        c = FL.case(seed)
        r = Row()
        r.seed = seed
        S, R, w, h = c.S, c.R, c.w, c.h
        shape = (len(c.rows), h, 3)
        # pin 1: one plain sub-ray is the frame depth_restatement folds -- at depth 3 the oracle's own (tests/test_fuzz_features.py)
        plain = LR.frame(LR.trails(c.ob, c.flat, c.ocam, LR.PLAIN, c.spp, 1, w, h, rows=c.rows), c.spp, c.depth)
        want = FF.deep_frame(c, c.depth)
        # (sum, avg and rgb: a lens frame's sum2 folds the squares of the sub-ray sums, the masked call's those of the samples)
        r.plain_pin = (same(plain[0].reshape(shape), want[0]) and same(plain[2].reshape(shape), want[2])
                       and np.array_equal(plain[3].reshape(shape), want[3]))
        # pin 2: under equal poses the shutter's rays are the lens's
        lens_rays = FL.rays(c, "lens")
        r.still_pin = same_rays(SHR.rays(c.still, c.time_jitter, c.lens, S, R, w, h), lens_rays)
        # pin 3: without time jitter sub-ray r is the lens's under the pose at r / R
        got = SHR.rays(c.motion, 0.0, c.lens, S, R, w, h)
        r.pose_pin = all(same_rays(tuple(a[r_] for a in got),
                                   tuple(a[0] for a in LR.rays(SHR.camera(c.motion, f32(r_) / f32(R)), c.lens, S, R, w, h, r_range=(r_, r_ + 1))))
                         for r_ in range(R))
        # pin 4: without a sky every sample of the case's lens frame is depth_restatement's
        tr = FL.trails(c, "lens")
        r.dark_pin = all(same(SR.radiance(t, c.depth, None), DR.radiance(DR.plain([t])[0], c.depth))
                         for per_pixel in tr for samples in per_pixel for t in samples)
        # the tables the guides gather from: the oracle's flat triangles give the bits of the product's own
        t, m = FF.product_bih(c).tris, FF.product_bih(c).materials
        with np.errstate(all="ignore"):
            nrm = np.cross(t["v1"] - t["v0"], t["v2"] - t["v0"]).astype(f32)
            nrm = nrm / np.sqrt((nrm * nrm).sum(-1, keepdims=True), dtype=f32)
            mine = (nrm, m["surf"][t["mat"]], m["emissive"][t["mat"]][:, None] * m["emit"][t["mat"]])
        r.tables_pin = all(same(np.asarray(a, f32), b) for a, b in zip(mine, FL.triangle_tables(c)))
        # coverage
        r.open, r.R, r.S = c.lens[1] > 0, R, S
        r.batches = len(FL.batches(c))
        r.batches_as_drawn = r.batches == (1 if c.fit is None else -(-R // c.fit))
        r.sharded = c.shard != FF.WHOLE
        r.odd = c.odd is not None
        r.non_finite = r.odd and not (np.isfinite(lens_rays[0]).all() and np.isfinite(lens_rays[1]).all())
        plain_o, plain_d, _ = LR.rays(c.ocam, LR.PLAIN, S, 1, w, h)
        plain_hits = LR.first_hits(c.ob, plain_o, plain_d)[0]
        r.sub_ray_hits_differ = bool((LR.first_hits(c.ob, lens_rays[0], lens_rays[1]) != plain_hits[None]).any())
        r.close_differs = bool((SHR.first_hits_at(c.ob, c.motion, 1.0, w, h) != SHR.first_hits_at(c.ob, c.motion, 0.0, w, h)).any())
        r.hit_and_miss = bool((plain_hits >= 0).any() and (plain_hits < 0).any())
        g1 = FL.guides(c, "first")
        assert np.array_equal(g1["tri"].reshape(-1), plain_hits)
        hit = g1["tri"] >= 0
        blank = (np.zeros((w, h, 3), f32), np.zeros((w, h), f32))          # what a step accepts does not depend on the colours
        lengths = [FL.temporal_want(c, previous, blank, blank, False)[1]["len"] for previous in FL.PREVIOUS]
        r.accepts = any(bool((n > 1).any()) for n in lengths)
        r.rejects = any(bool((hit & (n == 1)).any()) for n in lengths)
        r.behind = False
        for previous in FL.PREVIOUS:
            pos, rot = TR.camera(FL.camera_of(c, previous))
            with np.errstate(all="ignore"):
                e = g1["point"] - pos
                k0 = (e[..., 0] * rot[0] + e[..., 1] * rot[1]) + e[..., 2] * rot[2]
            r.behind |= bool((hit & ~(k0 > 0)).any())
        out.append(r)
    return out


PINS = (
    ("with LR.PLAIN and one sub-ray LR.frame is fuzz_features.deep_frame", "plain_pin"),
    ("under equal poses SHR.rays is LR.rays", "still_pin"),
    ("without time jitter a sub-ray is LR.sub_ray under SHR.camera(motion, r / R)", "pose_pin"),
    ("without a sky every sample is depth_restatement's", "dark_pin"),
    ("the oracle's flat triangles give the tables DeviceScene.guides gathers from", "tables_pin"),
    ("lens.workspace's arithmetic gives the drawn number of batches", "batches_as_drawn"),
)


@pytest.mark.parametrize("what, name", PINS, ids=[p[1] for p in PINS])
def test_pin_holds_on_every_seed(table, what, name):
    assert [r.seed for r in table if not getattr(r, name)] == [], what


def share(percent):
    return -(-len(SEEDS) * percent // 100)


COVERAGE = (
    ("the aperture is open", lambda r: r.open, share(40)),
    ("R > 1", lambda r: r.R > 1, share(50)),
    ("R == S with S > 1", lambda r: r.R == r.S and r.S > 1, share(10)),
    ("the dense frame runs in several batches", lambda r: r.batches > 1, share(30)),
    ("a shard other than the whole", lambda r: r.sharded, share(15)),
    ("an odd lens", lambda r: r.odd, share(5)),
    ("an odd lens that gives a non-finite ray", lambda r: r.non_finite, 1),
    ("a sub-ray's first hit differs from the plain ray's of its pixel", lambda r: r.sub_ray_hits_differ, share(30)),
    ("the close pose's first hits differ from the open pose's", lambda r: r.close_differs, share(30)),
    ("the frame has both a primary hit and a miss", lambda r: r.hit_and_miss, share(30)),
    ("the temporal step accepts history at some pixel", lambda r: r.accepts, share(30)),
    ("the temporal step rejects history at some hit pixel", lambda r: r.rejects, share(30)),
    ("a point lies behind the previous camera", lambda r: r.behind, 3),
)


@pytest.mark.parametrize("what, fact, least", COVERAGE, ids=[c[0] for c in COVERAGE])
def test_the_slice_covers(table, what, fact, least):
    count = sum(1 for r in table if fact(r))
    print(f"seeds {SEEDS[0]}..{SEEDS[-1]} where {what}: {count} (at least {least} asked)")
    assert count >= least, f"{what}: {count} seeds, {least} asked"
