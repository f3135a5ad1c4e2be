"""The inputs of tests/test_gpu_fuzz_image.py, judged without a GPU: on every seed of the slice the restatements the image stages are
held to agree with each other and with the oracle where they meet (a stride of 1, a glare of no levels, the reference curve, guides
without a hit), and the slice holds enough of every case the denoise, sparse, glare and film kernels and their drivers branch on,
counted from fuzz_image.case(seed), the oracle's guides and frame, and the restatements alone.

Measured: 19 s for the 400 seeds, most of it the three cameras' first-hit walks of case()."""
import numpy as np
import pytest

import denoise_restatement as DNR
import film_restatement as FR
import fuzz_image as FI
import fuzz_lens as FL
import glare_restatement as GR
import upsample_restatement as UR
from bitcmp import same

SEEDS = FI.SLICE
f32 = np.float32


class Row:
    pass


def normal_stop_splits(G, passes, squarings):
    """Whether some valid pixel has, in some pass, a valid tap inside the image whose normal weight is 0 and another whose is > 0:
    denoise_restatement.one_pass's t, tap for tap."""
    valid, nrm = G["tri"] >= 0, G["normal"]
    zeroed, kept = np.zeros(valid.shape, bool), np.zeros(valid.shape, bool)
    with np.errstate(all="ignore"):
        for i in range(passes):
            s = 1 << i
            for dy in (-2, -1, 0, 1, 2):
                for dx in (-2, -1, 0, 1, 2):
                    vq, inside = DNR.shifted(valid, dy * s, dx * s)
                    nq = DNR.shifted(nrm, dy * s, dx * s)[0]
                    dn = (nrm[..., 0] * nq[..., 0] + nrm[..., 1] * nq[..., 1]) + nrm[..., 2] * nq[..., 2]
                    t = np.where(dn > 0, dn, f32(0))
                    for _ in range(squarings):
                        t = t * t
                    ok = valid & inside & vq
                    zeroed |= ok & (t == 0)
                    kept |= ok & (t > 0)
    return bool((zeroed & kept).any())


def accepted_taps(G, s, oy, ox, sigma_p, cos_n):
    """How many of its four lattice neighbours every pixel accepts: upsample_restatement.gather's `acc`, tap for tap."""
    tri, nrm, pnt = G["tri"], G["normal"], G["point"]
    rows, cols = tri.shape
    yy, xx = np.mgrid[0:rows, 0:cols]
    yl, xl = (yy - oy) // s * s + oy, (xx - ox) // s * s + ox
    hit, n = tri >= 0, np.zeros((rows, cols), int)
    with np.errstate(all="ignore"):
        for j in (0, 1):
            for i in (0, 1):
                qy, qx = yl + j * s, xl + i * s
                inside = (qy >= 0) & (qy < rows) & (qx >= 0) & (qx < cols)
                gy, gx = np.clip(qy, 0, rows - 1), np.clip(qx, 0, cols - 1)
                q_hit, nq, d = tri[gy, gx] >= 0, nrm[gy, gx], pnt[gy, gx] - pnt
                dn = (nrm[..., 0] * nq[..., 0] + nrm[..., 1] * nq[..., 1]) + nrm[..., 2] * nq[..., 2]
                pd = (nrm[..., 0] * d[..., 0] + nrm[..., 1] * d[..., 1]) + nrm[..., 2] * d[..., 2]
                on_surface = q_hit & (dn >= f32(cos_n)) & (np.abs(pd) <= f32(sigma_p))
                n += inside & np.where(hit, on_surface, ~q_hit)
    return n


@pytest.fixture(scope="module")
def table(sqt, O):
    """One Row per seed: the pins and the facts the coverage conditions count."""
    out = []
    for seed in SEEDS:
        c = FI.case(seed)
        r = Row()
        r.seed = seed
        w, h = c.w, c.h
        clean = FL.guides(c, c.cam_name)
        G = FI.poisoned(c, clean)
        tri, nrm, pnt = G["tri"], G["normal"], G["point"]
        avg, rgb = FI.oracle_frame(c)
        counts = FI.want_counts(c)
        A = np.where((counts == c.ispp)[..., None], avg, f32(0)).astype(f32)          # what the masked render leaves where it is the dense frame
        X = FI.scaled(c, A)
        with np.errstate(all="ignore"):
            var = DNR.variance(A * f32(c.ispp), A * A * f32(c.ispp), counts)          # some variance: the pins below hold for any
        stops = FI.sparse_stops(c)
        # pin 1: with stride 1 every pixel is on the lattice
        ones = UR.sparse_mask(tri, nrm, pnt, 1, 0, 0, **stops)
        filled = UR.upsample(X, tri, nrm, pnt, ones, 1, 0, 0, var=var, **stops)
        r.stride_one_pin = bool((ones == 1).all()) and same(filled[0], X) and same(filled[1], var)
        # pin 2: no levels, gain 1, exposure 1
        r.no_glare_pin = same(GR.glare(X, 1.0, (1.0, 1.0, 1.0), levels=0), X)
        # pin 3: the reference curve is the oracle's tonemap
        r.reference_pin = np.array_equal(FR.develop(O, avg, curve="reference")[0], rgb)
        # pin 4: guides without a hit filter nothing
        none = np.full_like(tri, -1)
        got = DNR.denoise(X, none, nrm, pnt, var=var, **FI.filter_params(c))
        r.no_hit_pin = same(got[0], X) and same(got[1], var)
        # pin 5
        r.ceiling_pin = bool(f32(c.ceiling) > f32(c.threshold)) and bool(np.isfinite(f32(c.ceiling)))
        # coverage
        r.big, r.huge = max(w, h) > 16, max(w, h) > 64
        hit = clean["tri"] >= 0
        r.hit_and_miss = bool(hit.any() and (~hit).any())
        r.normal_stop = normal_stop_splits(G, c.passes, c.squarings)
        r.step_past_side, r.step_8 = (1 << (c.passes - 1)) >= min(w, h), (1 << (c.passes - 1)) >= 8
        mask = UR.sparse_mask(tri, nrm, pnt, c.stride, *c.offset, **stops)
        lattice = UR.lattice(w, h, c.stride, *c.offset)
        r.hole = bool(((mask != 0) & ~lattice).any())
        taps = accepted_taps(G, c.stride, *c.offset, **stops)
        assert bool((mask[taps == 0] != 0).all())                       # no accepted tap, no weight: the restatement traces the pixel
        r.few_taps = bool(((mask == 0) & (taps < 4)).any())
        r.stride_past_side = c.stride > min(w, h)
        r.counts_0_1_n = bool((counts == 0).any() and (counts == 1).any() and (counts > 1).any())
        r.poisoned = c.poisoned
        sizes = GR.level_sizes(w, h, c.levels)
        r.one_by_one_early = (1, 1) in sizes[:-1]
        r.no_levels = c.levels == 0
        x = GR.exposed(X, c.exposure, c.gain)
        r.odd_glare_input = bool((~np.isfinite(x) | (x < 0)).any())
        r.curve = c.curve
        hist = FR.histogram(X)
        r.no_slot = int(hist[1:FR.SLOTS - 1].sum()) == 0
        free = FR.expose(hist, None, **dict(c.meter, e_min=1e-45, e_max=3.4028235e38))
        r.at_e_min = not r.no_slot and bool(free < f32(c.meter["e_min"]))
        r.at_e_max = not r.no_slot and bool(free > f32(c.meter["e_max"]))
        r.sparse_and_film = c.t_sparse is not None and c.film_kind != "none"
        out.append(r)
    return out


PINS = (
    ("with stride 1 sparse_mask is all ones and upsample the identity", "stride_one_pin"),
    ("with levels 0, gain 1 and exposure 1 glare returns its input's bits", "no_glare_pin"),
    ("develop under the reference curve is the oracle's tonemap of its frame", "reference_pin"),
    ("on guides with tri = -1 everywhere denoise returns its inputs", "no_hit_pin"),
    ("the drawn ceiling is above the drawn threshold as float32, and finite", "ceiling_pin"),
)


@pytest.mark.parametrize("what, name", PINS, ids=[p[1] for p in PINS])
def test_pin_holds_on_every_seed(table, what, name):
    assert [r.seed for r in table if not getattr(r, name)] == [], what


def share(percent):
    return -(-len(SEEDS) * percent // 100)


COVERAGE = (
    ("a side is > 16", lambda r: r.big, share(40)),
    ("a side is > 64", lambda r: r.huge, share(5)),
    ("the frame has both a hit and a miss", lambda r: r.hit_and_miss, share(40)),
    ("some valid pixel has a valid tap the normal stop zeroes and another it keeps", lambda r: r.normal_stop, share(30)),
    ("the largest filter step reaches past the shorter side", lambda r: r.step_past_side, share(40)),
    ("the largest filter step is >= 8 (a forced tiled form falls back to direct)", lambda r: r.step_8, share(30)),
    ("the sparse mask has a hole", lambda r: r.hole, share(20)),
    ("an unset pixel has fewer than four accepted taps", lambda r: r.few_taps, share(30)),
    ("the stride exceeds a side", lambda r: r.stride_past_side, share(10)),
    ("the counts hold a 0, a 1 and a larger value", lambda r: r.counts_0_1_n, share(10)),
    ("the guides are poisoned", lambda r: r.poisoned, share(20)),
    ("the pyramid reaches 1 x 1 before its last level", lambda r: r.one_by_one_early, share(15)),
    ("levels = 0", lambda r: r.no_levels, share(5)),
    ("a glare input pixel is NaN, inf or negative after the gain", lambda r: r.odd_glare_input, share(15)),
) + tuple((f"the film curve is {curve}", (lambda r, curve=curve: r.curve == curve), share(10)) for curve in FR.CURVES) + (
    ("expose falls back: no slot is usable", lambda r: r.no_slot, 3),
    ("expose is clamped at e_min", lambda r: r.at_e_min, 3),
    ("expose is clamped at e_max", lambda r: r.at_e_max, 3),
    ("Temporal runs with sparse and film together", lambda r: r.sparse_and_film, share(15)),
)


@pytest.mark.parametrize("what, fact, least", COVERAGE, ids=[c[0] for c in COVERAGE])
def test_the_slice_covers(table, what, fact, least):
    count = sum(1 for r in table if fact(r))
    print(f"seeds {SEEDS[0]}..{SEEDS[-1]} where {what}: {count} (at least {least} asked)")
    assert count >= least, f"{what}: {count} seeds, {least} asked"
