"""Randomised parity campaign for what came after the frame campaign (tests/fuzz_gpu.py): caller-given path depth, caller-given
lights in every cast form, masked and multi-view calls, and the three ray queries, on the random scenes and cameras of
fuzz_gpu.make_scene / make_camera.  Seed N is the scene and camera that fuzz_gpu.run_case(N) renders: `case` makes the same first
draws from default_rng(N), and everything else a case needs comes from a second generator, default_rng([N, 1]), in the order written
in `case` (recorded seeds keep reproducing only while that order stays).

Expected values come from the C oracle (O.BIH.render, intersectBIH, the trick-camera raytrace / raycast of tests/ray_oracle.py,
O.tonemap) and from the two restatements that tests pin to it: tests/depth_restatement.py (any depth) and lights_restatement.Restatement
(any lights).  tests/test_fuzz_features.py pins both on every seed of the pytest slice and judges what the slice covers, without a GPU;
tests/test_gpu_fuzz_features.py runs the slice.  Every comparison is on bits with NaNs canonicalised, RGB8 exactly.

    python tests/fuzz_features.py [seconds=240] [first_seed=0]

prints one line per mismatch with the seed that reproduces it, and a summary.

Two conventions of the ray batch.  The oracle reaches a caller-given ray through a camera whose rotation adds +0 to each direction
component (tests/ray_oracle.py), so the radiance queries (raytrace, raycast) get the batch with every -0 direction component
made +0; `intersect`, whose oracle call takes the ray as it is, gets the batch unchanged.  And a ray batch's seeds have nothing to do
with the frame's: the camera rays in it are rays like any other."""
import functools
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)
import pyoracle as O  # noqa: E402

import fuzz_gpu as F  # noqa: E402
import depth_restatement as DR  # noqa: E402
import sky_restatement as SR  # noqa: E402
from bitcmp import canon, same  # noqa: E402
import f32_folds  # noqa: E402
from f32_folds import from_zero  # noqa: E402
from lights_restatement import Restatement, avg_of, fold_cast  # noqa: E402
from ray_oracle import check_hits, oracle_hits, oracle_raycast, oracle_raytrace, positive_zeros  # noqa: E402
from render_options import DEFAULT_SLOTS  # noqa: E402
from scenes import oracle_tris_of  # noqa: E402

sqt = importlib.import_module("squigly-trace_amd")      # importing the package loads no library: F.load_libraries does, when a case runs
f32 = np.float32
tonemaps = functools.partial(f32_folds.tonemaps, O)
DEPTHS = (1, 2, 4, 5, 8)
WHOLE = (None, 0, 1)
# frame sides 1 .. 16, the larger ones more often: a light has to light and to shadow a hit pixel of the frame to count as seen, and
# a path has to live to level 3 (tests/test_fuzz_features.py holds the slice to counts of both)
SIDES = np.arange(1, 17)
SIDE_WEIGHTS = np.where(SIDES >= 7, 3.0, 1.0) / np.where(SIDES >= 7, 3.0, 1.0).sum()


class Case:
    """One seed: scene, cameras, frame, depth, lights, mask, ray batch, options; and the oracle's tree of the scene."""


def light_pairs(table):
    return [(row[:3], row[3:]) for row in np.asarray(table, f32)]


def case(seed):
    c = Case()
    c.seed = seed
    rng = np.random.default_rng(seed)                                   # exactly fuzz_gpu.run_case's first draws
    c.v, c.mats, c.mat, c.scale = F.make_scene(rng)
    c.camt = F.make_camera(rng, c.scale)
    v, scale = c.v, c.scale
    c.ob = O.BIH(oracle_tris_of(O, v, c.mats, c.mat))
    c.flat = c.ob.flatten()
    c.ocam = O.camera_from_text(c.camt)

    rng = np.random.default_rng([seed, 1])                              # everything below: the second generator, in this order
    # 1. the frame
    c.w, c.h = int(rng.choice(SIDES, p=SIDE_WEIGHTS)), int(rng.choice(SIDES, p=SIDE_WEIGHTS))
    c.spp = int(rng.choice([1, 2, 3]))
    c.shard = WHOLE
    if rng.random() < 0.3 and c.w > 1:
        rb, ns = int(rng.choice([1, 2, 3, 8, 16])), int(rng.integers(2, 6))
        si = int(rng.integers(0, ns))
        c.shard = (rb, si if DR.shard_rows(c.w, (rb, si, ns)) else 0, ns)   # shard 0 always has rows
    c.rows = DR.shard_rows(c.w, c.shard)
    # 2. the depth
    c.depth = int(rng.choice(DEPTHS))
    # 3. the lights
    c.cam_rays = [O.make_ray(c.w, c.h, y, x, c.ocam) for y in range(c.w) for x in range(c.h)]
    prim = [c.ob.intersect(o, d) for o, d in c.cam_rays]
    points = [(h.point.x, h.point.y, h.point.z) for h in prim if h.hit]
    n_lights = int(rng.choice([1, 2, 3, 5]))
    lights = np.zeros((n_lights, 6), f32)
    for li in lights:
        li[:3] = (rng.uniform(-3, 3, 3) * scale).astype(f32)
        li[3:] = rng.uniform(0.2, 4, 3)
        odd = rng.random()
        if odd < 0.1 and points:
            li[:3] = points[int(rng.integers(0, len(points)))]          # dl = 0 at that pixel
        elif 0.1 <= odd < 0.2:
            li[int(rng.integers(0, 3))] = np.nan
        if rng.random() < 0.15:
            li[3 + int(rng.integers(0, 3))] = rng.choice([0.0, -1.5, np.inf])
    c.lights = lights
    # 4. the live mask of the masked call
    yy, xx = np.meshgrid(np.arange(len(c.rows)), np.arange(c.h), indexing="ij")
    c.live = ((yy + xx) % 2 == 0) if rng.random() < 0.5 else (rng.random((len(c.rows), c.h)) < 0.5)
    # 5. the second camera
    c.camt2 = F.make_camera(rng, scale)
    c.ocam2 = O.camera_from_text(c.camt2)
    # 6. the ray batch: the frame's camera rays, vertex-to-vertex rays, rays with special components
    o = [r[0] for r in c.cam_rays]
    d = [r[1] for r in c.cam_rays]
    flatv = v.reshape(-1, 3)
    for _ in range(int(rng.integers(0, 201))):
        a, b = flatv[int(rng.integers(0, len(flatv)))], flatv[int(rng.integers(0, len(flatv)))]
        with np.errstate(all="ignore"):
            o.append(a.copy())
            d.append((b - a).astype(f32))
    specials = np.array([0.0, -0.0, np.nan, np.inf, -np.inf], f32)
    for _ in range(int(rng.integers(0, 51))):
        ro = (rng.uniform(-2, 2, 3) * scale).astype(f32)
        rd = rng.normal(0, 1, 3).astype(f32)
        for _ in range(int(rng.integers(1, 4))):
            (ro if rng.random() < 0.4 else rd)[int(rng.integers(0, 3))] = specials[int(rng.integers(0, 5))]
        o.append(ro)
        d.append(rd)
    c.ray_o = np.ascontiguousarray(np.array(o, f32).reshape(-1, 3))
    c.ray_d = np.ascontiguousarray(np.array(d, f32).reshape(-1, 3))
    n = len(c.ray_o)
    s = np.empty(n, np.int64)                                           # small, above 2^40 and negative, by thirds (make_families)
    third = np.arange(n) % 3
    s[third == 0] = rng.integers(0, 1 << 20, int((third == 0).sum()))
    s[third == 1] = rng.integers(1 << 40, 1 << 60, int((third == 1).sum()))
    s[third == 2] = -rng.integers(1, 1 << 60, int((third == 2).sum()))
    c.ray_s = s
    # 7. kernel options: fuzz_gpu.run_case's, and the three of the newer pipelines
    c.knobs = {"pool": int(rng.integers(0, 2)), "resident": int(rng.integers(0, 2)), "refill_min": int(rng.choice([1, 8, 12, 33, 64])),
               "flush_min": int(rng.choice([0, 1, 40, 64])), "guided": int(rng.integers(0, 4)),
               "primary_resident": int(rng.integers(0, 2)), "pixel_major": int(rng.integers(0, 2)),
               "cull": int(rng.random() < 0.8), "descend_extra": int(rng.choice([0, 1, 2, 5])), "descend_lanes": int(rng.choice([1, 16, 40])),
               "primary_pooled": int(rng.random() < 0.25), "trace_blocks_per_cu": int(rng.integers(0, 4)),
               "lds_node_kb": int(rng.choice([0, 1, 4, 32]))}
    c.deep = int(rng.integers(0, 2))
    c.cast_wavefront = int(rng.integers(0, 2))
    c.slots = int(rng.choice([DEFAULT_SLOTS, c.w * c.h + 17]))          # the small one: samples and lights run in several batches
    c.knobs["level1_cull"] = int(rng.integers(0, 2))                    # the last draw of this step: the ones before it stay what they were
    return c


# ---- expected values ---------------------------------------------------------------------------------------------------------
def product_bih(c):
    if not hasattr(c, "bih"):
        tris = np.zeros(len(c.v), sqt._native.TRI_DTYPE)
        tris["v0"], tris["v1"], tris["v2"], tris["mat"] = c.v[:, 0], c.v[:, 1], c.v[:, 2], c.mat
        c.bih = sqt.BIH(sqt.Mesh.from_arrays(tris, c.mats))
    return c.bih


def frame_paths(c, second=False):
    """depth_restatement.frame_paths of the case's shard under its first or second camera, walked once to MAX_DEPTH: the walk
    sky_restatement keeps for the case, with each Miss read as None."""
    key = "_paths2" if second else "_paths"
    if not hasattr(c, key):
        setattr(c, key, [DR.plain(trails) for trails in SR.fuzz_frame_paths(c, second)])
    return getattr(c, key)


def deep_frame(c, depth, second=False):
    """(sum, sum2, avg, rgb8) [rows, h, 3] of the path-traced frame under `depth`."""
    s, q, avg = DR.fold_frame(frame_paths(c, second), depth)
    shape = (len(c.rows), c.h, 3)
    avg = avg.reshape(shape)
    return s.reshape(shape), q.reshape(shape), avg, tonemaps(avg)


def restatement(c):
    if not hasattr(c, "_R"):
        c._R = Restatement(O, c.ob)
    return c._R


def cast_frame(c, lights):
    """(avg, rgb8, T, lit) of the cast frame of the case's shard under `lights` (pairs): T [rows * h, 3] per primary ray."""
    rays = [c.cam_rays[y * c.h + x] for y in c.rows for x in range(c.h)]
    T, lit = restatement(c).radiance("frame", rays, lights)
    avg = avg_of(fold_cast(T, 0, c.spp), c.spp).reshape(len(c.rows), c.h, 3)
    return avg, tonemaps(avg), T, lit


def oracle_frame(c, cast):
    """O.BIH.render of the case's shard: (avg, rgb8)."""
    avg, rgb, _ = c.ob.render(c.ocam, c.spp, c.w, c.h, cast=cast)
    return avg[c.rows], rgb[c.rows]


def radiance_rays(c):
    """The batch as the radiance queries get it (module docstring)."""
    return c.ray_o, positive_zeros(c.ray_d), c.ray_s


def ray_paths(c):
    if not hasattr(c, "_ray_paths"):
        c._ray_paths = DR.plain(SR.fuzz_ray_paths(c))
    return c._ray_paths


# ---- one case on the GPU -----------------------------------------------------------------------------------------------------
DEVICE_ERROR = []      # the first HIP error of this process: after one, no case touches the device again


def run_case(seed):
    """Every check of the seed; returns the list of mismatch messages (empty: all equal).  A refusal is a mismatch."""
    import torch
    F.load_libraries()
    if DEVICE_ERROR:
        raise RuntimeError(f"not run: the device reported an error earlier in this process ({DEVICE_ERROR[0]})")
    c = case(seed)
    bad = []
    cam, cam2 = sqt.camera_from_text(c.camt), sqt.camera_from_text(c.camt2)
    w, h, spp, shard, D = c.w, c.h, c.spp, c.shard, c.depth
    rows = len(c.rows)
    dev = "cuda:0"
    ds = sqt.DeviceScene(product_bih(c), 0)

    def forms(variant, deep=0, cast_wavefront=0):
        ds.set_option("variant", variant)
        ds.set_option("deep", deep)
        ds.set_option("cast_wavefront", cast_wavefront)

    def frame_check(what, got, want_avg, want_rgb):
        torch.cuda.synchronize()
        avg, rgb = got[0].cpu().numpy(), got[1].cpu().numpy()
        if not same(avg, want_avg):
            bad.append(f"{what}: avg differs in {int((canon(avg) != canon(want_avg)).any(-1).sum())}/{rows * h} pixels")
        elif not np.array_equal(rgb, want_rgb):
            bad.append(f"{what}: rgb8 differs")
        if ds.last_plan()["launched"] != 1:
            bad.append(f"{what}: plan says launched = {ds.last_plan()['launched']}")

    try:
        for k, val in c.knobs.items():
            ds.set_option(k, val)
        ds.set_option("slots", c.slots)                                 # from the start: a workspace only grows
        # ---- depth
        for depth, deep in ((D, c.deep), (3, 1)):
            ds.set_depth(depth)
            _, _, want, want8 = deep_frame(c, depth)
            for variant in (2, 1):
                forms(variant, deep)
                frame_check(f"depth {depth} deep {deep} variant {variant}", ds.render_rows(cam, spp, w, h, shard=shard), want, want8)
            forms(2, deep)
            q = ds.raytrace(*ds.camera_rays(cam, w, h, shard=shard), seeds=sqt.frame_seeds(spp, w, h, shard=shard, device=dev),
                            samples=spp, want_rgb=True)
            frame_check(f"depth {depth} deep {deep} raytrace of the camera rays", (q.avg, q.rgb), want, want8)
        # ---- masked, under D
        ds.set_depth(D)
        forms(2, c.deep)
        want_s, want_q, want, want8 = deep_frame(c, D)
        live = c.live
        mask = torch.from_numpy(live.astype(np.uint8)).to(dev)
        sums = torch.full((rows, h, 3), 5.5, dtype=torch.float32, device=dev)
        sums2 = torch.full((rows, h, 3), -6.5, dtype=torch.float32, device=dev)
        counts = torch.full((rows, h), 77, dtype=torch.int32, device=dev)
        avg = torch.full((rows, h, 3), 8.25, dtype=torch.float32, device=dev)
        rgb = torch.full((rows, h, 3), 99, dtype=torch.uint8, device=dev)
        ds.render_rows_masked(cam, spp, w, h, 0, spp, sums, mask=mask, sums2=sums2, counts=counts, shard=shard, out_avg=avg, out_rgb=rgb)
        torch.cuda.synchronize()
        s, q2, n, a, r = (t.cpu().numpy() for t in (sums, sums2, counts, avg, rgb))
        if not (same(s[live], want_s[live]) and same(q2[live], want_q[live]) and (n[live] == spp).all()
                and same(a[live], want[live]) and np.array_equal(r[live], want8[live])):
            bad.append(f"masked call, depth {D}: a live pixel differs from the restatement's sum, sum2, count, avg or rgb")
        dead = ~live
        if not ((s[dead] == 5.5).all() and (q2[dead] == -6.5).all() and (n[dead] == 77).all() and (a[dead] == 8.25).all() and (r[dead] == 99).all()):
            bad.append(f"masked call, depth {D}: a dead pixel lost a sentinel")
        # ---- views, under D
        va, vr = ds.render_views([cam, cam2], spp, w, h, shard=shard)
        singles = [ds.render_rows(cm, spp, w, h, shard=shard) for cm in (cam, cam2)]
        torch.cuda.synchronize()
        for i, (sa, sr) in enumerate(singles):
            if not (same(va[i].cpu().numpy(), sa.cpu().numpy()) and torch.equal(vr[i], sr)):
                bad.append(f"views, depth {D}: view {i} differs from its single-view frame")
        _, _, want2, want28 = deep_frame(c, D, second=True)
        if not (same(va[1].cpu().numpy(), want2) and np.array_equal(vr[1].cpu().numpy(), want28)):
            bad.append(f"views, depth {D}: the second view differs from the restatement")
        # ---- lights
        pairs = light_pairs(c.lights)
        want, want8, T, _ = cast_frame(c, pairs)
        ds.set_lights(c.lights)
        for name, variant, wave in (("variant 1", 1, 0), ("per-lane", 2, 0), ("wavefront", 2, 1)):
            forms(variant, 0, wave)
            frame_check(f"cast frame under {len(pairs)} lights, {name}", ds.render_rows(cam, spp, w, h, cast=True, shard=shard), want, want8)
        forms(2, 0, c.cast_wavefront)
        rad = ds.raycast(*ds.camera_rays(cam, w, h, shard=shard))
        torch.cuda.synchronize()
        if not same(rad.cpu().numpy().reshape(-1, 3), T):                # a query stores T itself: no fold, a -0 stays -0
            bad.append(f"raycast of the camera rays under {len(pairs)} lights differs from the restatement")
        ds.set_lights(None)
        want, want8 = oracle_frame(c, cast=True)
        for name, variant, wave in (("variant 1", 1, 0), ("per-lane", 2, 0), ("wavefront", 2, 1)):
            forms(variant, 0, wave)
            frame_check(f"cast frame after set_lights(None), {name}", ds.render_rows(cam, spp, w, h, cast=True, shard=shard), want, want8)
        # ---- queries on the ray batch
        want_hits = oracle_hits(c.ob, c.ray_o, c.ray_d)
        ro, rd, rs = radiance_rays(c)
        want3 = from_zero(oracle_raytrace(O, c.ob, ro, rd, rs))
        wantD = from_zero(DR.radiances(ray_paths(c), D))
        # the oracle's cast render is 1 * (0 + T), which turns a -0 of T (a -0 surface colour) into +0, and the query stores T: the
        # restatement says T, and the oracle's value is held to 0 + T
        want_cast0 = oracle_raycast(O, c.ob, ro, rd)
        want_cast, _ = restatement(c).radiance("batch", list(zip(ro, rd)), [sqt.REFERENCE_LIGHT])
        if not same(from_zero(want_cast), want_cast0):
            bad.append("the lights restatement's 0 + T differs from the oracle's raycast on the ray batch")
        for name, variant in (("drawn form", 2), ("variant 1", 1)):
            forms(variant, c.deep, c.cast_wavefront)
            got = ds.intersect(c.ray_o, c.ray_d)
            torch.cuda.synchronize()
            try:
                check_hits(tuple(t.cpu().numpy() for t in got), want_hits, ("intersect", name))
            except AssertionError as e:
                bad.append(f"intersect, {name}: {e}")
            for depth, exp in ((3, want3), (D, wantD)):
                ds.set_depth(depth)
                got = ds.raytrace(ro, rd, seeds=rs).sum
                torch.cuda.synchronize()
                if not same(got.cpu().numpy(), exp):
                    bad.append(f"raytrace of {len(ro)} rays at depth {depth}, {name}: {int((canon(got.cpu().numpy()) != canon(exp)).any(-1).sum())} rays differ")
            got = ds.raycast(ro, rd)
            torch.cuda.synchronize()
            if not same(got.cpu().numpy(), want_cast) or not same(from_zero(got.cpu().numpy()), want_cast0):
                bad.append(f"raycast of {len(ro)} rays, {name}: {int((canon(got.cpu().numpy()) != canon(want_cast)).any(-1).sum())} rays differ")
    except sqt.SquiglyError as e:
        if " failed: " in str(e):                                       # a HIP error is no refusal: nothing more runs on this device
            DEVICE_ERROR.append(f"seed {seed}: {e}")
            raise
        bad.append(f"refused: {e}")
    except RuntimeError as e:                                           # torch's own report of a HIP error (a synchronize, a copy)
        if "HIP error" in str(e) or "CUDA error" in str(e):
            DEVICE_ERROR.append(f"seed {seed}: {e}")
        raise
    finally:
        ds.close()
    return bad


def describe(c):
    return (f"seed {c.seed}: {len(c.v)} tris, {c.w}x{c.h} @ {c.spp}, shard {c.shard}, depth {c.depth}, {len(c.lights)} lights, "
            f"{len(c.ray_o)} rays, deep {c.deep}, cast_wavefront {c.cast_wavefront}, slots {c.slots}, {c.knobs}")


def main(budget=240.0, seed=0):
    return F.campaign("fuzz_features", run_case, budget, seed)


if __name__ == "__main__":
    sys.exit(main(float(sys.argv[1]) if len(sys.argv) > 1 else 240.0, int(sys.argv[2]) if len(sys.argv) > 2 else 0))
