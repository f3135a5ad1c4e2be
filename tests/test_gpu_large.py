"""Frames and ray batches at the 32-bit index boundaries: every size here is derived from a type width -- a byte or
element offset that passes 2^31 or 2^32, a pixel count at INT32_MAX or at the wavefront form's 2^29 -- and is run once from the side
that is accepted and once from the side that is refused.  Every comparison is on bits.  The reference is the CPU oracle on a stated
subset of rows (the first 2, the last 2, the 2 at each boundary, 64 drawn with a fixed seed); the rest of a frame is held to a second
GPU render of the same rows as shards of fewer than 2^24 pixels, the size at which the other GPU tests tie the kernels to the oracle.
Nothing of frame size is copied to the host.

A test skips only when the device has less free memory than it needs (the formula is in the test, both numbers in the reason)."""
import ctypes as C
import os
import time

import numpy as np
import pytest

from bitcmp import ibits
from render_options import DEFAULT_SLOTS, THREADS

pytestmark = pytest.mark.gpu
f32 = np.float32
GB = 1 << 30
INT32_MAX = 2 ** 31 - 1
N_RANDOM_ROWS = 64


# ---- memory ----------------------------------------------------------------------------------------------------------------
def workspace_bytes(pixels, slots):
    """ensure_workspace: 32 B per pixel (px_pixel, t0, tri0, sum[3], mirror t and triangle), 33 B per slot and per pixel of the mirror
    rays' spare region (state, two ray quads), 12 B per slot (radiance), and the counters."""
    return 32 * pixels + 33 * (slots + pixels) + 12 * slots + (1 << 16)


def frame_slots(pixels, spp, opt_slots=DEFAULT_SLOTS):
    return max(pixels, min(opt_slots, pixels * spp))


def require_memory(need, what):
    import torch
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info(0)
    if free < need * 1.1:
        pytest.skip(f"{what}: needs {need / GB:.1f} GB x 1.1 of device memory, {free / GB:.1f} GB are free")


@pytest.fixture()
def scene(sqt, product_scene):
    """A device scene of the test's own: its workspace goes back to the driver when the test ends."""
    import torch
    assert sqt.device_count() >= 1, "no HIP device: the product has no CPU fallback"
    bih, cam, _ = product_scene
    ds = sqt.DeviceScene(bih, 0)
    t0 = time.time()
    yield ds, cam
    torch.cuda.synchronize()
    ds.close()
    sqt.release_cached_memory()
    torch.cuda.empty_cache()
    print(f"[large] {os.environ.get('PYTEST_CURRENT_TEST', '').split(' ')[0]}: {time.time() - t0:.1f} s")


# ---- rows ------------------------------------------------------------------------------------------------------------------
def checked_rows(w, h, boundaries, seed):
    """The rows held to the oracle: the first 2, the last 2, the row a boundary pixel index falls in and the one before it, and
    N_RANDOM_ROWS rows drawn with a fixed seed."""
    rows = {0, 1, w - 2, w - 1}
    for b in boundaries:
        assert 0 < b < w * h, (b, w, h)
        rows |= {b // h - 1, b // h}
    rng = np.random.default_rng(seed)
    rows |= set(int(y) for y in rng.choice(w, N_RANDOM_ROWS, replace=False))
    return sorted(y for y in rows if 0 <= y < w)


def oracle_row(ob, ocam, spp, w, h, y, cast):
    avg, rgb, _ = ob.render(ocam, spp, w, h, cast=cast, threads=THREADS, rows=(y, y + 1))
    return avg[0], rgb[0]


def bits_equal(t, a):
    """A device float32 tensor against a host float32 array, on bits."""
    import torch
    want = torch.from_numpy(ibits(a)).to(t.device)
    return bool(torch.equal(t.contiguous().view(torch.int32), want))


def shard_rows_index(sqt, w, sh, device):
    import torch
    L = sqt.lib()
    rows = L.sq_shard_rows(w, sh)
    j = torch.arange(rows, dtype=torch.int64, device=device)
    blk = j // sh.row_block
    return (blk * sh.n_shards + sh.shard) * sh.row_block + (j - blk * sh.row_block)


def small_shards(sqt, w, h):
    """Row blocks of 8 dealt to as many shards as keep every shard below 2^24 pixels."""
    n = 1
    L = sqt.lib()
    while L.sq_shard_rows(w, sqt.Shard(8, 0, n)) * h >= 1 << 24:
        n += 1
    return [sqt.Shard(8, i, n) for i in range(n)]


def equal_to_small_shards(sqt, ds, w, h, frames, render_shard, live=None):
    """Every shard of fewer than 2^24 pixels, rendered on its own by render_shard(shard tuple) -> tensors in the order of `frames`
    ([w, h, ...] device tensors), equals the same rows of the frames.  live: [w, h] mask of the pixels to compare (None = all)."""
    import torch
    shards = small_shards(sqt, w, h)
    assert all(sqt.lib().sq_shard_rows(w, sh) * h < 1 << 24 for sh in shards)
    for sh in shards:
        idx = shard_rows_index(sqt, w, sh, frames[0].device)
        parts = render_shard((sh.row_block, sh.shard, sh.n_shards))
        torch.cuda.synchronize()
        for k, (big, part) in enumerate(zip(frames, parts)):
            got = big[idx]
            if part.dtype == torch.float32:
                got, part = got.view(torch.int32), part.view(torch.int32)
            if live is not None:
                m = live[idx] != 0
                m = m[..., None] if got.dim() == 3 else m
                got, part = torch.where(m, got, torch.zeros_like(got)), torch.where(m, part, torch.zeros_like(part))
            if not torch.equal(got, part):
                bad = (got != part).nonzero()[:4].tolist()
                raise AssertionError(f"frame {k} differs from shard {sh.shard} of {sh.n_shards} at (local row, column, channel) {bad}")
    return len(shards)


def set_form(ds, variant, slots=DEFAULT_SLOTS):
    for k, v in {"variant": variant, "resident": 1, "profile": 0, "overlap": 0, "primary_pooled": 0, "pool": 1, "slots": slots}.items():
        ds.set_option(k, v)


# ---- 1. RGB8 at INT32_MAX pixels: byte offsets past 2^31 and 2^32 --------------------------------------------------------------
@pytest.mark.parametrize("cast", [True, False], ids=["cast", "variant1"])
def test_rgb8_frame_just_under_int32_max_pixels(sqt, scene, oracle_scene, cast):
    """46340 x 46340 = 2 147 395 600 pixels, the largest square frame a call takes (46341^2 > 2^31 - 1): the byte offset pix * 3 of a
    pixel passes 2^31 at pixel 715 827 883 and 2^32 at pixel 1 431 655 766.  Per-pixel kernel, d_rgb only (6.4 GB), 1 spp."""
    import torch
    ds, cam = scene
    ob, ocam, _ = oracle_scene
    w = h = 46340
    assert w * h <= INT32_MAX < (w + 1) * (h + 1)
    require_memory(w * h * 3 + (1 << 24) * 3 + (2 << 30), "d_rgb of 46340 x 46340 and one shard")
    set_form(ds, 1)
    rgb = torch.full((w, h, 3), 123, dtype=torch.uint8, device="cuda:0")
    _, got = ds.render_rows(cam, 1, w, h, cast=cast, want_avg=False, out_rgb=rgb)
    torch.cuda.synchronize()
    assert ds.last_plan()["trace_form"] == "per_pixel" and ds.last_plan()["launched"] == 1
    for y in checked_rows(w, h, [1 << 24, (2 ** 31 + 2) // 3, (2 ** 32 + 2) // 3], seed=46340 + cast):
        want = torch.from_numpy(oracle_row(ob, ocam, 1, w, h, y, cast)[1]).cuda()
        assert torch.equal(rgb[y], want), f"row {y} differs from the oracle"
    n = equal_to_small_shards(sqt, ds, w, h, [rgb], lambda sh: [ds.render_rows(cam, 1, w, h, cast=cast, shard=sh, want_avg=False)[1]])
    assert n >= 128
    del rgb, got


# ---- 2. float3 frames: byte offsets past 2^32 -------------------------------------------------------------------------------
W2, H2 = 18919, 18921               # 357 966 399 pixels: pix * 12 passes 2^32 at pixel 357 913 942 (row 18916), odd h: edge tiles
assert W2 * H2 > (2 ** 32 + 11) // 12 > (W2 - 3) * H2


@pytest.mark.parametrize("variant", [1, 2], ids=["variant1", "wavefront"])
def test_float3_frame_past_2_32_bytes(sqt, scene, oracle_scene, variant):
    """d_avg (4.3 GB) of 18919 x 18921 pixels at 1 spp through the per-pixel kernel and through the default wavefront form, whose
    workspace (110 B per pixel at one slot per pixel: 39 GB) is indexed by slot and active-pixel numbers up to 3.6e8."""
    import torch
    ds, cam = scene
    ob, ocam, _ = oracle_scene
    w, h = W2, H2
    px = w * h
    need = px * 12 + (1 << 24) * 12 + (2 << 30) + (workspace_bytes(px, frame_slots(px, 1)) if variant == 2 else 0)
    require_memory(need, f"d_avg of {w} x {h}" + (" and the wavefront workspace" if variant == 2 else ""))
    set_form(ds, variant)
    avg = torch.full((w, h, 3), -3.5, dtype=torch.float32, device="cuda:0")
    ds.render_rows(cam, 1, w, h, want_rgb=False, out_avg=avg)
    torch.cuda.synchronize()
    plan = ds.last_plan()
    assert plan["launched"] == 1 and plan["trace_form"] == ("per_pixel" if variant == 1 else "resident")
    for y in checked_rows(w, h, [1 << 24, (2 ** 31 + 11) // 12, (2 ** 32 + 11) // 12], seed=W2 + variant):
        assert bits_equal(avg[y], oracle_row(ob, ocam, 1, w, h, y, False)[0]), f"row {y} differs from the oracle"
    equal_to_small_shards(sqt, ds, w, h, [avg], lambda sh: [ds.render_rows(cam, 1, w, h, shard=sh, want_rgb=False)[0]])
    del avg


# ---- 3. float element offsets past 2^31, the range call in two steps ---------------------------------------------------------
def test_range_call_past_2_31_float_elements(sqt, scene, oracle_scene):
    """26755 x 26757 = 715 883 535 pixels: the element offset pix * 3 passes 2^31 at pixel 715 827 883 (row 26752).  variant 1, 2 spp
    as the ranges [0, 1) and [1, 2): d_sum carries the fold between the calls, d_avg is the 2-sample frame (17 GB together)."""
    import torch
    ds, cam = scene
    ob, ocam, _ = oracle_scene
    w, h = 26755, 26757
    px = w * h
    assert px > (2 ** 31 + 2) // 3 > (w - 3) * h
    require_memory(2 * px * 12 + 2 * (1 << 24) * 12 + (2 << 30), f"d_avg and d_sum of {w} x {h}")
    set_form(ds, 1)
    avg = torch.full((w, h, 3), -3.5, dtype=torch.float32, device="cuda:0")
    sums = torch.full((w, h, 3), 7.25, dtype=torch.float32, device="cuda:0")
    ds.render_rows_range(cam, 2, w, h, 0, 1, sums, want_rgb=False, out_avg=avg)
    ds.render_rows_range(cam, 2, w, h, 1, 2, sums, want_rgb=False, out_avg=avg)
    torch.cuda.synchronize()
    for y in checked_rows(w, h, [(2 ** 32 + 11) // 12, (2 ** 31 + 2) // 3], seed=26755):
        assert bits_equal(avg[y], oracle_row(ob, ocam, 2, w, h, y, False)[0]), f"row {y} differs from the oracle"

    def shard(sh):
        rows = sqt.lib().sq_shard_rows(w, sqt.Shard(*sh))
        s = torch.empty((rows, h, 3), dtype=torch.float32, device="cuda:0")
        ds.render_rows_range(cam, 2, w, h, 0, 1, s, shard=sh, want_rgb=False)
        a, _ = ds.render_rows_range(cam, 2, w, h, 1, 2, s, shard=sh, want_rgb=False)
        return [a, s]
    equal_to_small_shards(sqt, ds, w, h, [avg, sums], shard)
    del avg, sums


# ---- 4. the wavefront form's limit: 2^29 pixels ---------------------------------------------------------------------------
@pytest.mark.parametrize("slots", [DEFAULT_SLOTS, 1 << 29], ids=["default_slots", "slots_2_29"])
def test_wavefront_frame_past_2_29_pixels_is_refused(sqt, scene, slots):
    """23171 x 23173 = 536 941 583 pixels > 2^29: the audit puts the wavefront form's limit at 2^29 pixels, so the
    call is refused with the documented words before any device work, and no buffer is touched; the per-pixel kernel takes the frame
    (test_range_call_past_2_31_float_elements is larger)."""
    import torch
    ds, cam = scene
    w, h = 23171, 23173
    assert w * h > 1 << 29
    set_form(ds, 2, slots)
    L = sqt.lib()
    avg = torch.full((4, 4, 3), -3.5, dtype=torch.float32, device="cuda:0")
    rgb = torch.full((4, 4, 3), 123, dtype=torch.uint8, device="cuda:0")
    sums = torch.full((4, 4, 3), 7.25, dtype=torch.float32, device="cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    sh = sqt.Shard(w, 0, 1)
    want = sqt.frame_size_error(w, h, wavefront=True)
    assert "2^29" in want
    rc = L.sq_render_rows_device(ds._h, C.byref(cam), 1, w, h, 0, sh, avg.data_ptr(), rgb.data_ptr(), stream)
    assert rc != 0
    assert L.sq_last_error().decode() == want
    rc = L.sq_render_rows_device_range(ds._h, C.byref(cam), 2, w, h, 0, sh, 0, 1, sums.data_ptr(), avg.data_ptr(), rgb.data_ptr(), stream)
    assert rc != 0
    assert L.sq_last_error().decode() == want
    with pytest.raises(sqt.SquiglyError) as e:
        ds.render_rows(cam, 1, w, h)
    assert str(e.value) == want
    torch.cuda.synchronize()
    assert bool((avg == -3.5).all()) and bool((rgb == 123).all()) and bool((sums == 7.25).all())
    # a launch has at most 2^32 - 1 threads, and the per-lane primary pass has one per tile lane: a frame one pixel wide enumerated
    # 64 pixels of a row per wave (primary_tiles 0) pads every pixel to 64 lanes, so 2^26 x 1 pixels would be a launch of 2^32 threads
    ds.set_option("primary_resident", 0)
    ds.set_option("primary_tiles", 0)
    rc = L.sq_render_rows_device(ds._h, C.byref(cam), 1, 1 << 26, 1, 0, sqt.Shard(1 << 26, 0, 1), avg.data_ptr(), rgb.data_ptr(), stream)
    ds.set_option("primary_resident", 1)
    ds.set_option("primary_tiles", 1)
    assert rc != 0
    assert b"image too large for one launch of the primary rays" in L.sq_last_error()
    assert ds.last_plan()["launched"] == 0 and ds.last_plan()["primary_form"] == "per_lane"
    torch.cuda.synchronize()
    assert bool((avg == -3.5).all()) and bool((rgb == 123).all())
    # exactly 2^29 pixels is inside the limit: 16384 x 32768, rendered in test_wavefront_frame_of_2_29_pixels
    assert sqt.frame_size_error(1 << 14, 1 << 15, wavefront=True) is None


def test_wavefront_frame_of_2_29_pixels(sqt, scene, oracle_scene):
    """The accepted side of the same limit: 16384 x 32767 = 536 838 144 pixels <= 2^29 (one more row passes it), odd h.  Default
    wavefront form, 1 spp, d_rgb only: the active-pixel list, the slots and the mirror rays' region behind them reach 2^29 entries,
    3 x (active pixel) reaches 1.61e9 and the trace kernel's queue 2^30 positions (59 GB of workspace)."""
    import torch
    ds, cam = scene
    ob, ocam, _ = oracle_scene
    w, h = 16384, 32767
    px = w * h
    assert px <= 1 << 29 < (w + 1) * h
    require_memory(px * 3 + (1 << 24) * 3 + (2 << 30) + workspace_bytes(px, frame_slots(px, 1)), f"d_rgb of {w} x {h} and the wavefront workspace")
    set_form(ds, 2)
    rgb = torch.full((w, h, 3), 123, dtype=torch.uint8, device="cuda:0")
    ds.render_rows(cam, 1, w, h, want_avg=False, out_rgb=rgb)
    torch.cuda.synchronize()
    assert ds.last_plan()["trace_form"] == "resident"
    for y in checked_rows(w, h, [1 << 24, 1 << 28], seed=16384):
        want = torch.from_numpy(oracle_row(ob, ocam, 1, w, h, y, False)[1]).cuda()
        assert torch.equal(rgb[y], want), f"row {y} differs from the oracle"
    equal_to_small_shards(sqt, ds, w, h, [rgb], lambda sh: [ds.render_rows(cam, 1, w, h, shard=sh, want_avg=False)[1]])
    del rgb


# ---- 5. the masked call at the float3 boundary ----------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [1, 2], ids=["variant1", "wavefront"])
def test_masked_call_past_2_32_bytes(sqt, scene, oracle_scene, variant):
    """18919 x 18921, mask = every 97th pixel and the whole last row, 1 spp: dead pixels keep their sentinel in d_avg, d_sum, d_sum2
    and d_count; a live pixel holds the oracle's sample (sum = avg = r, sum2 = r * r rounded, count = 1)."""
    import torch
    ds, cam = scene
    ob, ocam, _ = oracle_scene
    w, h = W2, H2
    px = w * h
    need = 3 * px * 12 + px * 4 + px + 3 * px + (3 << 30) + (workspace_bytes(px, frame_slots(px, 1)) + px * 12 if variant == 2 else 0)
    require_memory(need, f"three float3 buffers, counts and mask of {w} x {h}" + (" and the wavefront workspace" if variant == 2 else ""))
    set_form(ds, variant)
    dev = "cuda:0"
    mask = torch.zeros(px, dtype=torch.uint8, device=dev)
    mask[::97] = 1
    mask[-h:] = 200
    mask = mask.view(w, h)
    avg = torch.full((w, h, 3), -3.5, dtype=torch.float32, device=dev)
    sums = torch.full((w, h, 3), 7.25, dtype=torch.float32, device=dev)
    sums2 = torch.full((w, h, 3), 5.5, dtype=torch.float32, device=dev)
    counts = torch.full((w, h), 77, dtype=torch.int32, device=dev)
    ds.render_rows_masked(cam, 1, w, h, 0, 1, sums, mask=mask, sums2=sums2, counts=counts, want_rgb=False, out_avg=avg)
    torch.cuda.synchronize()
    live = mask != 0
    assert int(live.sum()) == ((w - 1) * h + 96) // 97 + h            # the multiples of 97 before the last row, and the last row
    for t, sent in ((avg, -3.5), (sums, 7.25), (sums2, 5.5)):
        assert bool(((t == sent).all(-1) | live).all()), "a dead pixel was written"
    assert torch.equal(counts, torch.where(live, torch.ones_like(counts), torch.full_like(counts, 77)))
    for y in checked_rows(w, h, [1 << 24, (2 ** 31 + 11) // 12, (2 ** 32 + 11) // 12], seed=97 + variant):
        r = oracle_row(ob, ocam, 1, w, h, y, False)[0]
        m = live[y][:, None]
        for t, ref, sent in ((avg, r, -3.5), (sums, r, 7.25), (sums2, (r * r).astype(f32), 5.5)):
            want = torch.where(m, torch.from_numpy(np.ascontiguousarray(ref, f32)).cuda(), torch.full((h, 3), sent, dtype=torch.float32, device=dev))
            assert torch.equal(t[y].view(torch.int32), want.view(torch.int32)), f"row {y} differs from the oracle"
    # every live pixel of the frame against unmasked renders of small shards (sum = avg = the one sample)
    equal_to_small_shards(sqt, ds, w, h, [avg, sums], lambda sh: [ds.render_rows(cam, 1, w, h, shard=sh, want_rgb=False)[0]] * 2, live=mask)
    del avg, sums, sums2, counts, mask, live


# ---- 6. the stopping rule above 2^31 / 3 pixels -----------------------------------------------------------------------------
def test_adaptive_update_past_2_31_float_elements(sqt, scene):
    """n = 715 827 883 + 1000 pixels: 3 * p passes 2^31 inside d_sum and d_sum2.  The inputs are a 4096-pixel pattern of hand-made
    statistics, tiled; the mask and the live count are the numpy restatement (rule_reference) of the pattern, tiled."""
    import torch
    ds, _ = scene
    n = (2 ** 31 + 2) // 3 + 1000
    assert n == 715827883 + 1000
    P = 4096
    tiles, tail = divmod(n, P)
    require_memory((tiles + 1) * P * (12 + 12 + 4 + 1) + n * 3 + (2 << 30), f"sums, sums2, counts and mask of {n} pixels")
    rng = np.random.default_rng(4096)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, 1e-38, 3e38, 1.0, 100.0, 4097.0], f32)
    counts = rng.choice(np.array([0, 1, 2, 3, 8, 64, 1000], np.int32), P)
    r = ((rng.random((P, 64, 3)) < 0.3) * rng.uniform(0, 100, (P, 64, 3))).astype(f32)
    keep = (np.arange(64)[None, :] < np.minimum(counts, 64)[:, None])[..., None]
    s = (r * keep).sum(1, dtype=f32)
    q = (r * r * keep).sum(1, dtype=f32)
    odd = rng.random((P, 3)) < 0.1
    s[odd] = special[rng.integers(0, len(special), odd.sum())]
    odd = rng.random((P, 3)) < 0.1
    q[odd] = special[rng.integers(0, len(special), odd.sum())]
    mask = rng.choice(np.array([0, 1, 1, 200], np.uint8), P)
    tol, eps = 0.5, 1.0
    want = sqt.rule_reference(s, q, counts, mask, tol, eps)
    assert 0 < want.sum() < (mask != 0).sum()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()              # noqa: E731
    ps, pq, pc, pm = up(s), up(q), up(counts), up(mask)
    ts, tq = ps.repeat(tiles + 1, 1)[:n], pq.repeat(tiles + 1, 1)[:n]
    tc, tm = pc.repeat(tiles + 1)[:n], pm.repeat(tiles + 1)[:n]
    live = ds.adaptive_update(ts, tq, tc, tm, tol, eps)
    assert live == tiles * int(want.sum()) + int(want[:tail].sum())
    pw = torch.where(up(want) != 0, pm, torch.zeros_like(pm))           # a converged pixel's byte is cleared, a live one keeps its byte
    assert bool((tm[:tiles * P].view(tiles, P) == pw[None]).all()) and torch.equal(tm[tiles * P:], pw[:tail])
    for t, p in ((ts.view(torch.int32), ps.view(torch.int32)), (tq.view(torch.int32), pq.view(torch.int32)), (tc, pc)):
        assert bool((t[:tiles * P].view((tiles, P) + tuple(p.shape[1:])) == p[None]).all()) and torch.equal(t[tiles * P:], p[:tail]), "an input was written"
    # the launch-size refusal, from both sides of it, with nothing launched: 2^32 - 256 pixels would be one launch of 2^24 - 1 workgroups
    L = sqt.lib()
    one = C.c_void_p(ts.data_ptr())
    assert L.sq_adaptive_update_device(ds._h, 2 ** 32 - 255, one, one, one, 0.5, 1.0, one, one, None) != 0
    assert b"too many pixels" in L.sq_last_error()
    del ts, tq, tc, tm


# ---- 7. camera rays -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,shard", [(W2, H2, (None, 0, 1)), (46340, 46340, (8, 3, 8))], ids=["18919x18921", "shard_of_46340x46340"])
def test_camera_rays_past_2_32_bytes(sqt, O, scene, oracle_scene, w, h, shard):
    """sq_camera_rays_device is 64-bit throughout (no limit but memory): origins and directions of 18919 x 18921 pixels (8.6 GB),
    and of one shard of eight of 46340 x 46340, against pyoracle.make_ray."""
    import torch
    ds, cam = scene
    _, ocam, _ = oracle_scene
    sh = sqt.Shard(w if shard[0] is None else shard[0], shard[1], shard[2])
    rows = sqt.lib().sq_shard_rows(w, sh)
    px = rows * h
    assert px * 12 > 2 ** 31
    require_memory(2 * px * 12 + (2 << 30), f"origins and directions of {rows} x {h} pixels")
    o, d = ds.camera_rays(cam, w, h, shard=shard)
    torch.cuda.synchronize()
    pos = torch.tensor(list(cam.pos), dtype=torch.float32, device="cuda:0")
    assert bool((o.view(torch.int32) == pos.view(torch.int32)).all()), "an origin is not the camera's position"
    bounds = [b for b in (1 << 24, (2 ** 31 + 11) // 12, (2 ** 32 + 11) // 12) if b < px]
    full = sorted({0, rows - 1} | {b // h for b in bounds})
    rng = np.random.default_rng(w + shard[1])
    some = sorted(set(int(j) for j in rng.choice(rows, N_RANDOM_ROWS, replace=False)) - set(full))
    gy = shard_rows_index(sqt, w, sh, "cpu").tolist()
    for j, cols in [(j, range(h)) for j in full] + [(j, range(int(rng.integers(0, 61)), h, 61)) for j in some]:
        cols = list(cols)
        want = np.array([O.make_ray(w, h, gy[j], x, ocam)[1] for x in cols], f32)
        assert bits_equal(d[j][torch.tensor(cols, device="cuda:0")], want), f"local row {j} (image row {gy[j]}) differs from make_ray"
    del o, d


# ---- 8. ray queries ----------------------------------------------------------------------------------------------------------
BLOCK = 1 << 20
_BLOCK = {}


def ray_block(sqt, ds, cam, ob, bih):
    """2^20 rays and the oracle's answer to each: the primary rays of a 1024 x 946 frame and the ray families of
    tests/test_gpu_rays.py (free space, on surfaces, axis-aligned and on split planes, degenerate)."""
    import torch
    from ray_oracle import make_families, oracle_hits
    if "rays" not in _BLOCK:
        fam = make_families(bih, 20)
        fo = np.concatenate([fam[k][0] for k in sorted(fam)]).astype(f32)
        fd = np.concatenate([fam[k][1] for k in sorted(fam)]).astype(f32)
        co, cd = ds.camera_rays(cam, 1024, 946)
        n_cam = BLOCK - len(fo)
        assert 0 < n_cam <= 1024 * 946
        o = np.concatenate([co.view(-1, 3)[:n_cam].cpu().numpy(), fo])
        d = np.concatenate([cd.view(-1, 3)[:n_cam].cpu().numpy(), fd])
        tri, dist, _ = oracle_hits(ob, o, d)
        dist = np.where(tri >= 0, dist, f32(np.inf)).astype(f32)
        assert 0 < (tri >= 0).sum() < len(tri)
        _BLOCK["rays"] = (o, d, tri.astype(np.int32), dist)
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in _BLOCK["rays"])


def tiled_equal(t, block, n, floats=False):
    """t[:n] is `block` repeated; floats: on bits, any two NaNs counting as equal (x86 and gfx950 NaN payloads differ)."""
    import torch
    tiles, tail = divmod(n, len(block))
    for a, b in ((t[:tiles * len(block)].view((tiles, len(block)) + tuple(block.shape[1:])), block[None]), (t[tiles * len(block):n], block[:tail])):
        eq = a.view(torch.int32) == b.view(torch.int32) if floats else a == b
        if floats:
            eq |= torch.isnan(a) & torch.isnan(b)
        if not bool(eq.all()):
            return False
    return True


def test_ray_query_past_one_lane_chunk(sqt, scene, oracle_scene, product_scene):
    """n = 2^30 + 12345 rays through the per-lane kernel (variant 1), which runs launches of 2^30 rays: the second launch starts at
    byte offset 12 * 2^30 of d_org and d_dir.  d_dist and d_point are NULL (30 GB of ray and result arrays)."""
    import torch
    ds, cam = scene
    ob, _, _ = oracle_scene
    n = (1 << 30) + 12345
    tiles = n // BLOCK + 1
    require_memory(tiles * BLOCK * 28 + (3 << 30), f"origins, directions and triangles of {n} rays")
    set_form(ds, 1)
    bo, bd, btri, _ = ray_block(sqt, ds, cam, ob, product_scene[0])
    o, d = bo.repeat(tiles, 1)[:n], bd.repeat(tiles, 1)[:n]
    tri = torch.full((n + 64,), -7, dtype=torch.int32, device="cuda:0")
    hits = ds.intersect(o, d, want_dist=False, want_point=False, out=(tri[:n], None, None))
    torch.cuda.synchronize()
    assert hits.dist is None and hits.point is None
    assert ds.last_plan()["trace_form"] == "per_pixel"
    assert tiled_equal(tri, btri, n), "a ray's triangle differs from the oracle's"
    assert bool((tri[n:] == -7).all()), "written past the last ray"
    del o, d, tri


@pytest.mark.parametrize("slots", [DEFAULT_SLOTS, (1 << 20) + 1], ids=["default_slots", "slots_2_20_plus_1"])
def test_ray_query_default_form_past_2_32_bytes(sqt, scene, oracle_scene, product_scene, slots):
    """n = 357 913 942 + 4099 rays through the default form (staged into the workspace slots, one level of the trace kernel): one chunk
    with the default `slots`, 342 chunks of 2^20 + 1 rays otherwise, whose offsets into d_org / d_dir pass 2^32 bytes."""
    import torch
    ds, cam = scene
    ob, _, _ = oracle_scene
    n = (2 ** 32 + 11) // 12 + 4099
    tiles = n // BLOCK + 1
    require_memory(tiles * BLOCK * 24 + n * 8 + (3 << 30) + workspace_bytes(1, min(slots, n)), f"rays and results of {n} rays and {min(slots, n)} slots")
    set_form(ds, 2, slots)
    bo, bd, btri, bdist = ray_block(sqt, ds, cam, ob, product_scene[0])
    o, d = bo.repeat(tiles, 1)[:n], bd.repeat(tiles, 1)[:n]
    tri = torch.full((n + 64,), -7, dtype=torch.int32, device="cuda:0")
    dist = torch.full((n + 64,), -3.5, dtype=torch.float32, device="cuda:0")
    ds.intersect(o, d, want_point=False, out=(tri[:n], dist[:n], None))
    torch.cuda.synchronize()
    assert ds.last_plan()["trace_form"] == "resident"
    assert tiled_equal(tri, btri, n), "a ray's triangle differs from the oracle's"
    assert tiled_equal(dist, bdist, n, floats=True), "a ray's distance differs from the oracle's"
    assert bool((tri[n:] == -7).all()) and bool((dist[n:] == -3.5).all()), "written past the last ray"
    del o, d, tri, dist


# ---- 9. refusals -------------------------------------------------------------------------------------------------------------
def test_single_view_calls_refuse_more_than_int32_max_pixels(sqt, scene, product_scene, oracle_scene, monkeypatch):
    """46341 x 46341 = 2 147 488 281 pixels > 2^31 - 1 on every single-view entry point, in every form: an error code, the same words
    as the Python layer's, and no buffer touched.  The same frame as one shard of two is inside the limit and renders."""
    import torch
    ds, cam = scene
    ob, ocam, _ = oracle_scene
    L = sqt.lib()
    w = h = 46341
    assert w * h > INT32_MAX
    dev = "cuda:0"
    B = {"avg": torch.full((4, 4, 3), -3.5, dtype=torch.float32, device=dev), "rgb": torch.full((4, 4, 3), 123, dtype=torch.uint8, device=dev),
         "sums": torch.full((4, 4, 3), 7.25, dtype=torch.float32, device=dev), "sums2": torch.full((4, 4, 3), 5.5, dtype=torch.float32, device=dev),
         "counts": torch.full((4, 4), 77, dtype=torch.int32, device=dev), "mask": torch.full((4, 4), 1, dtype=torch.uint8, device=dev)}
    keep = {k: v.clone() for k, v in B.items()}
    p = {k: v.data_ptr() for k, v in B.items()}
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    sh = sqt.Shard(w, 0, 1)
    want = sqt.frame_size_error(w, h)
    assert want == "46341 x 46341 pixels exceed 2^31 - 1 pixels in one call"
    for variant, cast in ((1, 0), (2, 0), (2, 1)):
        set_form(ds, variant)
        rc = L.sq_render_rows_device(ds._h, C.byref(cam), 1, w, h, cast, sh, p["avg"], p["rgb"], stream)
        assert rc != 0
        assert L.sq_last_error().decode() == want
        rc = L.sq_render_rows_device_range(ds._h, C.byref(cam), 2, w, h, cast, sh, 0, 1, p["sums"], p["avg"], p["rgb"], stream)
        assert rc != 0
        assert L.sq_last_error().decode() == want
        rc = L.sq_render_rows_device_masked(ds._h, C.byref(cam), 2, w, h, cast, sh, 0, 1, p["mask"], p["sums"], p["sums2"], p["counts"],
                                            p["avg"], p["rgb"], stream)
        assert rc != 0
        assert L.sq_last_error().decode() == want
        rc = L.sq_render_views_device(ds._h, C.byref(cam), 1, 1, w, h, cast, sh, 0, 1, p["sums"], p["avg"], p["rgb"], stream)
        assert rc != 0
        assert L.sq_last_error().decode() == want
        with pytest.raises(sqt.SquiglyError) as e:
            ds.render_rows(cam, 1, w, h, cast=bool(cast))
        assert str(e.value) == want
    # the one-shot call: the whole frame on one device is one shard
    monkeypatch.setenv("SQ_DEVICES", "0")
    out = np.full(48, 123, np.uint8)
    bih = product_scene[0]
    rc = L.sq_render_rgb8(C.byref(bih.scene), C.byref(cam), 1, w, h, 1, out.ctypes.data)
    assert rc != 0
    assert L.sq_last_error().decode() == "device 0 (shard 0 of 1): " + want
    rc = L.sq_render_f32(C.byref(bih.scene), C.byref(cam), 1, 23171, 23173, 0, out.ctypes.data)
    assert rc != 0
    assert L.sq_last_error().decode() == "device 0 (shard 0 of 1): " + sqt.frame_size_error(23171, 23173, wavefront=True)
    assert (out == 123).all()
    torch.cuda.synchronize()
    for k in B:
        assert torch.equal(B[k], keep[k]), k
    # accepted: one shard of two of the same frame (23173 rows x 46341 columns = 1 073 859 993 pixels), cast, d_rgb only
    rows = L.sq_shard_rows(w, sqt.Shard(8, 0, 2))
    assert rows * h <= INT32_MAX
    require_memory(rows * h * 3 + (2 << 30), f"d_rgb of one shard of two of {w} x {h}")
    set_form(ds, 1)
    _, rgb = ds.render_rows(cam, 1, w, h, cast=True, shard=(8, 0, 2), want_avg=False)
    torch.cuda.synchronize()
    gy = shard_rows_index(sqt, w, sqt.Shard(8, 0, 2), "cpu").tolist()
    assert gy[0] == 0 and gy[-1] == w - 1
    for j in (0, 1, rows - 2, rows - 1):
        wantrow = torch.from_numpy(oracle_row(ob, ocam, 1, w, h, gy[j], True)[1]).cuda()
        assert torch.equal(rgb[j], wantrow), f"local row {j} (image row {gy[j]}) differs from the oracle"
    del rgb
