"""The table of generator words of a resident scene (option "rng_table_mb"): its entries are the oracle's
generator words, and a frame that reads them is, bit for bit, the frame that computes them (rng_table_mb = 0) -- `avg` compared
as raw bits, `rgb` as bytes -- in every kind of call that reaches sq_gen_bounce1."""
import numpy as np
import pytest
import torch

from bitcmp import same_exact as same
from conftest import GOLDEN
from scenes import ROTATED

pytestmark = pytest.mark.gpu
DEFAULT_MB = 24576
MB = 1 << 20
HEADLINE = (1920, 1080, 256)          # rows, columns, samples
TILTED = b"0.5 6.5 1\n1.3 -0.2 0.1\n"


@pytest.fixture()
def ds(sqt, product_scene):
    bih, _, _ = product_scene
    d = sqt.DeviceScene(bih)
    yield d
    d.close()


@pytest.fixture(scope="module")
def cam(product_scene):
    return product_scene[1]


def on_off(ds, call, mb=DEFAULT_MB):
    """call() with the table (budget mb) and without it; both results, copied."""
    def run():
        out = call()
        torch.cuda.synchronize()
        return tuple(None if t is None else t.clone() for t in out)
    ds.set_option("rng_table_mb", mb)
    on = run()
    ds.set_option("rng_table_mb", 0)
    off = run()
    ds.set_option("rng_table_mb", mb)
    return on, off


def assert_covers(sqt, ds, w, h, samples, mb=DEFAULT_MB):
    """The scene's table holds what the frame can use under the budget (so the call above did read it)."""
    want = sqt.lib().sq_rng_table_cover(w, h, samples, mb * MB)
    assert want > 0 and ds.rng_table()[0] >= want


def test_golden_frame(sqt, ds, cam):
    on, off = on_off(ds, lambda: ds.render_rows(cam, 4, 64, 64))
    assert same(on, off)
    assert_covers(sqt, ds, 64, 64, 4)
    want = np.load(GOLDEN + "/scene_64x64_4spp_avg.npy")
    assert np.array_equal(on[0].cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert np.array_equal(on[1].cpu().numpy(), np.load(GOLDEN + "/scene_64x64_4spp_rgb8.npy"))


@pytest.mark.parametrize("samples", [3, 6])
def test_unaligned_runs(sqt, ds, cam, samples):
    """samples = 3: the seed rows start at every residue mod 4, and the only run is short; samples = 6: residues 0 and 2, a
    whole run and a short one."""
    on, off = on_off(ds, lambda: ds.render_rows(cam, samples, 40, 72))
    assert same(on, off)
    assert_covers(sqt, ds, 40, 72, samples)
    if samples == 3:
        want = np.load(GOLDEN + "/scene_40x72_3spp_avg.npy")
        assert np.array_equal(on[0].cpu().numpy().view(np.uint32), want.view(np.uint32))


def test_range_call_from_sample_5(sqt, ds, cam):
    w, h, n = 48, 56, 16

    def call():
        sums = torch.empty((w, h, 3), dtype=torch.float32, device="cuda")
        ds.render_rows_range(cam, n, w, h, 0, 5, sums)
        avg, rgb = ds.render_rows_range(cam, n, w, h, 5, n, sums)                 # k_base = 5: runs start at seed % 4 == 1
        return avg, rgb, sums
    on, off = on_off(ds, call)
    assert same(on, off)
    assert_covers(sqt, ds, w, h, n)
    assert same(on[:2], tuple(t.clone() for t in ds.render_rows(cam, n, w, h)))   # ... and it is the frame of one call


def test_shard_2_of_8(sqt, ds, cam):
    w, h, n = 96, 80, 8
    on, off = on_off(ds, lambda: ds.render_rows(cam, n, w, h, shard=(2, 2, 8)))
    assert same(on, off)
    assert_covers(sqt, ds, w, h, n)                                               # the whole frame's seeds: a shard has global rows
    whole = ds.render_rows(cam, n, w, h)[0]
    rows = [sqt.lib().sq_shard_global_row(j, sqt.Shard(2, 2, 8)) for j in range(on[0].shape[0])]
    assert same(on[0], whole[rows].contiguous())


def test_three_views(sqt, ds, cam):
    w, h, n = 56, 64, 12
    cams = [cam, sqt.camera_from_text(ROTATED), sqt.camera_from_text(TILTED)]
    on, off = on_off(ds, lambda: ds.render_views(cams, n, w, h))
    assert same(on, off)
    assert_covers(sqt, ds, w, h, n)
    for i, c in enumerate(cams):
        assert same((on[0][i].contiguous(), on[1][i].contiguous()), ds.render_rows(c, n, w, h))


def test_masked_call(sqt, ds, cam):
    w, h, n = 64, 48, 16
    g = torch.Generator().manual_seed(7)
    mask0 = (torch.rand((w, h), generator=g) < 0.6).to(torch.uint8)
    mask1 = (mask0.bool() & (torch.rand((w, h), generator=g) < 0.5)).to(torch.uint8)

    def call():
        sums = torch.zeros((w, h, 3), dtype=torch.float32, device="cuda")
        sums2 = torch.zeros((w, h, 3), dtype=torch.float32, device="cuda")
        counts = torch.zeros((w, h), dtype=torch.int32, device="cuda")
        avg = torch.zeros((w, h, 3), dtype=torch.float32, device="cuda")
        rgb = torch.zeros((w, h, 3), dtype=torch.uint8, device="cuda")
        ds.render_rows_masked(cam, n, w, h, 0, 6, sums, mask=mask0.cuda(), sums2=sums2, counts=counts, out_avg=avg, out_rgb=rgb)
        ds.render_rows_masked(cam, n, w, h, 6, n, sums, mask=mask1.cuda(), sums2=sums2, counts=counts, out_avg=avg, out_rgb=rgb)
        return avg, rgb, sums, sums2, counts
    on, off = on_off(ds, call)
    assert same(on, off)
    assert_covers(sqt, ds, w, h, n)
    assert int((on[4] == n).sum()) == int(mask1.sum()) and int((on[4] == 6).sum()) == int((mask0.bool() & ~mask1.bool()).sum())


@pytest.mark.parametrize("samples", [64, 37])
def test_few_pixels_split_the_samples(sqt, ds, cam, samples):
    """16 x 16 pixels: the launch has more workgroup rows (gridDim.y = min(samples, 64)) than a pixel has runs, so every
    blockIdx.y takes one run of four or none; 37 samples end in a run of one."""
    on, off = on_off(ds, lambda: ds.render_rows(cam, samples, 16, 16))
    assert same(on, off)
    assert_covers(sqt, ds, 16, 16, samples)


def test_half_covered_frame(sqt, ds, cam):
    """A budget of about half the frame's seeds: the pixels below the boundary read, those above compute, and the boundary
    falls inside an image row (waves with both kinds of lanes)."""
    w, h, n = 512, 512, 16
    full = sqt.lib().sq_rng_table_cover(w, h, n, DEFAULT_MB * MB)
    mb = 25
    half = sqt.lib().sq_rng_table_cover(w, h, n, mb * MB)
    assert full == w * h * n and 0.45 * full < half < 0.55 * full and half == mb * MB // 12
    assert (half // n) % w not in (0, w - 1)                                      # the first uncovered pixel is inside a row
    on, off = on_off(ds, lambda: ds.render_rows(cam, n, w, h), mb=mb)
    assert same(on, off)
    assert ds.rng_table()[0] >= half


def test_growth(sqt, product_scene, cam):
    """A second, larger frame after a small one: the table grows, and both frames are the computed ones."""
    sqt.release_cached_memory()                                                   # no table left over from an earlier scene
    d = sqt.DeviceScene(product_scene[0])
    try:
        assert d.rng_table()[0] == 0
        small = tuple(t.clone() for t in d.render_rows(cam, 4, 32, 32))
        c0 = d.rng_table()[0]
        assert c0 == 32 * 32 * 4
        large = tuple(t.clone() for t in d.render_rows(cam, 8, 128, 128))
        c1, words = d.rng_table(c0 - 8, 16)                                       # entries on both sides of the old end
        assert c1 == 128 * 128 * 8
        again = tuple(t.clone() for t in d.render_rows(cam, 4, 32, 32))            # the small frame reads the larger table
        d.set_option("rng_table_mb", 0)
        assert same(small, d.render_rows(cam, 4, 32, 32)) and same(again, small)
        assert same(large, d.render_rows(cam, 8, 128, 128))
        assert np.array_equal(words, sqt.debug_eval("tfgen3", np.arange(c0 - 8, c0 + 8)))
    finally:
        d.close()


def test_raytrace_seeds_inside_negative_and_huge(sqt, ds, cam):
    """One batch of radiance queries whose seed rows lie inside the table, across its end, below zero and above 2^32."""
    w, h, n = 128, 128, 8
    ds.render_rows(cam, n, w, h)                                                  # a query never builds a table: the frame does
    cover = ds.rng_table()[0]
    assert cover >= w * h * n
    o, d = ds.camera_rays(cam, w, h)
    k = 5                                                                         # samples per ray: rows of 5 seeds, every alignment
    m = w * h
    rng = np.random.default_rng(11)
    seeds = np.empty(m, np.int64)
    seeds[0::4] = rng.integers(0, cover - k, len(seeds[0::4]))
    seeds[1::4] = -rng.integers(1, 2 ** 40, len(seeds[1::4]))
    seeds[2::4] = 2 ** 32 + rng.integers(0, 2 ** 40, len(seeds[2::4]))
    seeds[3::4] = cover - k + rng.integers(-3, 8, len(seeds[3::4]))               # the last rows inside, and rows across the end
    seeds[:8] = [0, cover - k, cover - k + 1, cover - 1, cover, -1, -k, 2 ** 32]
    sd = torch.from_numpy(seeds).reshape(w, h)
    on, off = on_off(ds, lambda: ds.raytrace(o, d, seeds=sd, samples=k, want_rgb=True))
    assert same(on, off)
    assert ds.rng_table()[0] == cover                                             # ... and the query left the table as it was


def test_headline_table_and_frame(sqt, O, ds, cam):
    """The headline frame, once with the table and once without; and the headline-size table's entries against the oracle's
    generator words: the first 4096, the last 4096 and 4096 seeded-random positions."""
    w, h, n = HEADLINE
    ds.set_option("rng_table_mb", DEFAULT_MB)
    on = tuple(t.clone() for t in ds.render_rows(cam, n, w, h))
    torch.cuda.synchronize()
    cover = ds.rng_table()[0]
    assert cover >= sqt.lib().sq_rng_table_cover(w, h, n, DEFAULT_MB * MB) == 943503360
    head = sqt.lib().sq_rng_table_cover(w, h, n, DEFAULT_MB * MB)                # the headline-size table (a larger kept one has it as a prefix)
    rng = np.random.default_rng(20261016)
    picks = np.sort(rng.integers(0, head, 4096))
    got = {"first": ds.rng_table(0, 4096)[1], "last": ds.rng_table(head - 4096, 4096)[1],
           "random": np.stack([ds.rng_table(int(s), 1)[1][0] for s in picks])}
    seeds = {"first": np.arange(4096), "last": np.arange(head - 4096, head), "random": picks}
    for name in got:
        want = np.array([O.tfgen_words(int(s))[:3] for s in seeds[name]], np.uint32)
        assert np.array_equal(got[name], want), name
    ds.set_option("rng_table_mb", 0)
    off = ds.render_rows(cam, n, w, h)
    torch.cuda.synchronize()
    assert same(on, off)
