"""The kernel walk: a list of small calls whose union launches every GPU kernel of the library that a call can reach, each held bit
for bit to the oracle or its pinned restatements, and the list of the kernels no call can reach.

Belongs here: CASES (pure data: importing this module loads no library), what each case claims to launch, how a case runs and what it
is compared with.  tests/test_gpu_kernel_walk.py runs the cases; tools/kernel_walk_trace.py runs `main` under a kernel trace and
records which kernels each case dispatched (tests/golden/kernel_walk.json); tests/test_kernel_walk.py holds the library's kernel list
to that file plus UNREACHABLE, on the CPU.

A kernel is named by the demangled spelling of its instantiation up to its argument list (`short_name`): "sq_rng_fill",
"sq_primary<unsigned int, 0, true, Sky>".  What selects the template arguments (sq_device.hip: launch_frame, intersect_rays; sq_plan_call.h:
plan_call): StackT by the scene's index width (data/scene.obj: 2-byte stack words; scenes.tall_u32 of it: 4-byte), SRC by the call
(0 a camera frame, 1 render_views, 2 raytrace / raycast), AD by a masked call, Sky / DeepSky by set_sky, and the body by the variant,
the depth, the lights and the cast_wavefront / primary_* options.  A case names those keys, its claims follow from them (`claims`
below), and it asserts the plan it was written for: a case that silently takes another form fails.

Expected values come from the base scene: the padding of tall_u32 adds no triangle.  Depth 3 without a sky is O.BIH.render and the
oracle's trick-camera queries (ray_oracle), and the restatements are asserted equal to them here as well; other depths and skies are
sky_restatement, caller-given lights lights_restatement.  Every comparison is on bits with NaNs canonicalised (bitcmp), RGB8 exactly.

Workspaces only grow, so the order of the cases of one scene matters to the batches they run in: option "slots" is each call's
pixel count, the single-view and ray cases come first (a 19 x 21 frame at 3 spp then runs three batches of one sample per pixel: `last`
is 0 and 1), the multi-view cases after them.

    python tests/kernel_walk.py RESULT.json

runs every case once, each behind a one-element debug_eval whose argument is the case's index, and writes what passed."""
import functools
import importlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)
import pyoracle as O  # noqa: E402

import masked_calls as MC  # noqa: E402
import render_options as RO  # noqa: E402
import scenes as SC  # noqa: E402
import sky_restatement as SR  # noqa: E402
from bitcmp import canon, same  # noqa: E402
from f32_folds import fold_list, from_zero, tonemaps  # noqa: E402
from lights_restatement import Restatement, avg_of, fold_cast  # noqa: E402
from ray_oracle import check_hits, family_free, oracle_hits, oracle_raycast, oracle_raytrace, positive_zeros  # noqa: E402

sqt = importlib.import_module("squigly-trace_amd")      # importing the package loads no library
f32 = np.float32
# rows, columns, samples.  F8: whole tiles in one block.  FE: edge tiles both ways, two blocks of pixels, three batches.  F370: the
# narrow frame whose edge tiles are mostly padding; by the reference's makeRay (x offsets are divided by the row count) its pixels
# look past the scene, so it is the frame of primary misses -- black without a sky, the sky's gradient under one -- and of a
# pipeline without an active pixel.  tests/test_kernel_walk.py judges what the three frames show.
F8, FE, F370 = (8, 8, 2), (19, 21, 3), (3, 70, 3)
SKY = SR.GRADIENT
TYPE = {"u16": "unsigned short", "u32": "unsigned int"}
WORD = {"u16": 2, "u32": 4}
U32_HEIGHT = 23                                         # the tallest 4-byte tree sq_trace_rays_dense takes (tests/test_gpu_limits.py, EXPECT)
N_FREE_RAYS = 40
DEBUG_ROWS = 600                                        # more than one workgroup: a marker is a debug launch of exactly one
BIG_COLUMNS = 256                                       # the frames of sq_accumulate<false, *>: (n_cu + 1) rows of 256 pixels


def lights_of(n):
    """n point lights inside the room, each with a power of its own per channel."""
    return [((0.4 * i - 0.8, 3.0 - 0.3 * i, -1.0 + 0.2 * i), (2.0, 1.0 + 0.25 * i, 0.5 + 0.5 * i)) for i in range(n)]


def short_name(demangled):
    """A kernel's demangled name up to its argument list, without `void` and the anonymous namespace."""
    s = demangled.replace("(anonymous namespace)::", "").strip()
    s = s[5:] if s.startswith("void ") else s
    depth = 0
    for i, ch in enumerate(s):
        depth += (ch == "<") - (ch == ">")
        if ch == "(" and depth == 0:
            return s[:i]
    return s


# ---- the kernels no call can reach (tests/test_kernel_walk.py proves it through sq_plan_call) -----------------------------------------
# 4-byte stack words mean at least 0x8000 branches or triangles; the resident layout then needs at least 1 MiB of branch quads or
# 256 KiB of triangle records, against 160 KiB of LDS, so the planner never chooses the resident form for such a scene.
UNREACHABLE = tuple(sorted(
    [f"sq_trace_rays<unsigned int, true, 1024, {prof}, {pool}>" for prof in ("false", "true") for pool in ("false", "true")]
    + [f"sq_primary_resident<unsigned int, {src}{sky}>" for src in ("0, false", "0, true", "1, false", "2, false") for sky in ("", ", Sky")]))


# ---- claims: the kernels a case's keys select ----------------------------------------------------------------------------------
def b(v):
    return "true" if v else "false"


def trace_kernel(scene, form, pool, profile):
    if form == "streaming_six_wave":
        return f"sq_trace_rays_dense<{TYPE[scene]}>"
    res = form == "resident"
    return f"sq_trace_rays<{TYPE[scene]}, {b(res)}, {1024 if res else 512}, {b(profile)}, {b(pool)}>"


def primary_kernels(scene, primary, src, ad, sky):
    k = ", Sky" if sky else ""
    if primary == "resident":
        return [f"sq_primary_resident<{TYPE[scene]}, {src}, {b(ad)}{k}>"]
    if primary == "per_lane":
        return [f"sq_primary<{TYPE[scene]}, {src}, {b(ad)}{k}>"]
    return [f"sq_primary_gen<{src}, {b(ad)}>", f"sq_primary_store<{b(ad)}{k}>"]


class Case:
    """One call: the scene, what is called (`kind`), the frame, the options over render_options.RADIANCE, the scene state, the plan it
    must take and the kernels it claims."""

    def __init__(self, name, scene, kind, claims, frame=None, opts=None, depth=3, sky=None, lights=None, cast=False, cast_wavefront=0,
                 plan=None, fresh=False):
        self.name, self.scene, self.kind, self.claims, self.frame = name, scene, kind, tuple(sorted(set(claims))), frame
        self.opts, self.depth, self.sky, self.lights, self.cast, self.cast_wavefront = dict(opts or {}), depth, sky, lights, cast, cast_wavefront
        self.plan, self.fresh = plan, fresh

    def __repr__(self):
        return self.name


def _cases():
    out = []

    def add(*a, **kw):
        out.append(Case(*a, **kw))

    def slots_of(frame, kind):
        w, h, _ = frame
        return {"views": 2 * w * h, "raytrace": w * h + N_FREE_RAYS, "raycast": w * h + N_FREE_RAYS}.get(kind, w * h)

    def kind_of(src, ad, cast):
        return {0: "masked" if ad else "render", 1: "views", 2: "raycast" if cast else "raytrace"}[src]

    def wave(name, scene, src, body, frame, opts=None, form=None, pool=1, profile=0, primary=None, ad=False, depth=3, sky=False, lights=None):
        """A call in the wavefront form.  body: "pipeline" (depth 3), "deep" (another depth, option deep, or a sky) or "cast"."""
        form = form or {"u16": "resident", "u32": "streaming_six_wave"}[scene]
        default_primary = "resident" if form == "resident" else "per_lane"
        primary = primary or default_primary
        opts = dict(opts or {})
        if primary == "pooled":
            opts["primary_pooled"] = 1
        elif primary != default_primary:
            opts["primary_resident"] = 0
        cast = body == "cast"
        kind = kind_of(src, ad, cast)
        claims = primary_kernels(scene, primary, src, ad, sky and not cast)
        if body == "pipeline":
            claims += [f"sq_gen_bounce1<{src}>", f"sq_shade1<{src}>", f"sq_mirror1_gen<{src}>", "sq_mirror1_store", f"sq_accumulate<true, {b(ad)}>"]
        elif body == "deep":
            claims += ["sq_deep_fold<DeepSky>" if sky else "sq_deep_fold<>"]
            if depth >= 2:
                claims += [f"sq_deep_gen<{src}>", f"sq_deep_bounce<{src}{', DeepSky' if sky else ''}>"]
        else:
            claims += [f"sq_cast_gen<{src}>", f"sq_cast_fold<{src}>"]
        if body != "deep" or depth >= 2 or primary == "pooled":
            claims.append(trace_kernel(scene, form, pool, profile))
        if src == 1:
            claims.append("sq_stage_cams")
        if lights:
            claims.append("sq_stage_lights")
        opts.setdefault("slots", slots_of(frame, kind))
        add(name, scene, kind, claims, frame=frame, opts=opts, depth=depth, sky=SKY if sky else None, lights=lights, cast=cast,
            cast_wavefront=int(cast),
            plan={"variant": 2, "stack_word_bytes": WORD[scene], "trace_form": form, "primary_form": primary, "launched": 1})

    def lane(name, scene, src, body, frame, ad=False, depth=3, sky=False, lights=None):
        """A call in the per-lane form (variant 1; a cast frame under caller-given lights in any variant)."""
        t, k = TYPE[scene], ", Sky" if sky else ""
        kernel = {"plain": f"sq_render_pixels<{t}, {src}, {b(ad)}>", "deep": f"sq_render_pixels_deep<{t}, {src}, {b(ad)}{k}>",
                  "cast": f"sq_cast_pixels<{t}, {src}, {b(ad)}>"}[body]
        claims = [kernel] + (["sq_stage_cams"] if src == 1 else []) + (["sq_stage_lights"] if lights else [])
        cast = body == "cast"
        variant = 2 if cast else 1
        add(name, scene, kind_of(src, ad, cast), claims, frame=frame, opts={"variant": variant}, depth=depth, sky=SKY if sky else None,
            lights=lights, cast=cast,
            plan={"variant": variant, "stack_word_bytes": WORD[scene], "trace_form": "per_pixel", "primary_form": "none", "launched": 1})

    # 1. every trace kernel under the three-level pipeline of a camera frame
    TRACE = {"u16": (("resident", {}, "resident", 1, 0), ("resident_pool0", {"pool": 0}, "resident", 0, 0),
                     ("resident_profile", {"profile": 1}, "resident", 1, 1), ("resident_profile_pool0", {"profile": 1, "pool": 0}, "resident", 0, 1),
                     ("dense", {"resident": 0}, "streaming_six_wave", 1, 0),
                     ("plain", {"resident": 0, "trace_blocks_per_cu": 1}, "streaming_plain", 1, 0),
                     ("plain_pool0", {"resident": 0, "pool": 0}, "streaming_plain", 0, 0),
                     ("plain_profile", {"resident": 0, "profile": 1}, "streaming_plain", 1, 1),
                     ("plain_profile_pool0", {"resident": 0, "profile": 1, "pool": 0}, "streaming_plain", 0, 1)),
             "u32": (("dense", {}, "streaming_six_wave", 1, 0), ("plain", {"trace_blocks_per_cu": 1}, "streaming_plain", 1, 0),
                     ("plain_pool0", {"pool": 0}, "streaming_plain", 0, 0), ("plain_profile", {"profile": 1}, "streaming_plain", 1, 1),
                     ("plain_profile_pool0", {"profile": 1, "pool": 0}, "streaming_plain", 0, 1))}
    for scene in ("u16", "u32"):
        for i, (tname, opts, form, pool, profile) in enumerate(TRACE[scene]):
            wave(f"{scene}_trace_{tname}", scene, 0, "pipeline", FE if i % 2 == 0 else F8, opts=opts, form=form, pool=pool, profile=profile)
    # 2. the wavefront bodies by source, mask and sky, with each scene's own primary form; the deep kernels at depths 1, 2, 4 and 8
    SOURCES = ((0, False, "frame"), (0, True, "masked"), (1, False, "views"), (2, False, "rays"))
    for scene in ("u16", "u32"):
        for i, (src, ad, sname) in enumerate(SOURCES):
            frame = FE if i % 2 == 0 else F8
            wave(f"{scene}_{sname}_pipeline", scene, src, "pipeline", frame, ad=ad)
            wave(f"{scene}_{sname}_deep{(2, 4, 8, 2)[i]}", scene, src, "deep", frame, ad=ad, depth=(2, 4, 8, 2)[i])
            wave(f"{scene}_{sname}_deep{(4, 8, 2, 4)[i]}_sky", scene, src, "deep", frame, ad=ad, depth=(4, 8, 2, 4)[i], sky=True)
        wave(f"{scene}_frame_deep1", scene, 0, "deep", F8, depth=1)
        wave(f"{scene}_frame_deep1_sky", scene, 0, "deep", F8, depth=1, sky=True)
        wave(f"{scene}_frame_deep3_sky", scene, 0, "deep", F8, depth=3, sky=True)
        wave(f"{scene}_frame_3x70_pipeline", scene, 0, "pipeline", F370)
        wave(f"{scene}_masked_3x70_deep4_sky", scene, 0, "deep", F370, ad=True, depth=4, sky=True)
        wave(f"{scene}_views_3x70_deep2_sky", scene, 1, "deep", F370, depth=2, sky=True)
    wave("u16_frame_3x70_primary_per_lane_sky", "u16", 0, "deep", F370, primary="per_lane", depth=8, sky=True)
    for scene in ("u16", "u32"):
        lane(f"{scene}_frame_3x70_variant1_deep4_sky", scene, 0, "deep", F370, depth=4, sky=True)
    # 3. the resident scene's per-lane primary pass ...
    for i, (src, ad, sname) in enumerate(SOURCES):
        wave(f"u16_{sname}_primary_per_lane", "u16", src, "pipeline", F8 if i % 2 == 0 else FE, primary="per_lane", ad=ad)
        wave(f"u16_{sname}_primary_per_lane_sky", "u16", src, "deep", F8 if i % 2 == 0 else FE, primary="per_lane", ad=ad, depth=(8, 1, 4, 2)[i], sky=True)
    # ... and the pooled one
    for src, ad, sname, sky in ((0, False, "frame", False), (0, False, "frame", True), (0, True, "masked", False), (0, True, "masked", True),
                                (1, False, "views", True), (2, False, "rays", False)):
        wave(f"u16_{sname}_primary_pooled{'_sky' if sky else ''}", "u16", src, "deep" if sky else "pipeline", FE, primary="pooled", ad=ad,
             depth=4 if sky else 3, sky=sky)
    wave("u32_masked_primary_pooled_sky", "u32", 0, "deep", F8, primary="pooled", ad=True, depth=2, sky=True)
    # 4. the per-lane form: variant 1 at depth 3, at other depths and under a sky, and cast under caller-given lights
    for scene in ("u16", "u32"):
        for i, (src, ad, sname) in enumerate(SOURCES):
            frame = F8 if i % 2 == 0 else FE
            lane(f"{scene}_{sname}_variant1", scene, src, "plain", frame, ad=ad)
            lane(f"{scene}_{sname}_variant1_deep{(1, 2, 4, 8)[i]}", scene, src, "deep", frame, ad=ad, depth=(1, 2, 4, 8)[i])
            lane(f"{scene}_{sname}_variant1_deep{(4, 8, 1, 3)[i]}_sky", scene, src, "deep", frame, ad=ad, depth=(4, 8, 1, 3)[i], sky=True)
            lane(f"{scene}_{sname}_cast_lights{(3, 5, 3, 5)[i]}", scene, src, "cast", frame, ad=ad, lights=(3, 5, 3, 5)[i])
    # 5. cast in the wavefront form: the lights take the samples' place, in two or more batches
    for scene, src, sname, n, frame in (("u16", 0, "frame", 5, FE), ("u16", 1, "views", 3, F8), ("u16", 2, "rays", 5, F8), ("u32", 0, "frame", 3, FE),
                                        ("u16", 0, "frame_reference_light", None, F8)):
        wave(f"{scene}_{sname}_cast_wavefront", scene, src, "cast", frame, lights=n)
    # 6. intersection queries
    for scene, form in (("u16", "resident"), ("u32", "streaming_six_wave")):
        add(f"{scene}_intersect", scene, "intersect", ["sq_rays_stage", "sq_rays_store", trace_kernel(scene, form, 1, 0)], frame=FE,
            opts={"slots": 64}, plan={"variant": 2, "stack_word_bytes": WORD[scene], "trace_form": form, "primary_form": "none", "launched": 1})
        add(f"{scene}_intersect_variant1", scene, "intersect", [f"sq_intersect_lanes<{TYPE[scene]}>"], frame=FE, opts={"variant": 1},
            plan={"variant": 1, "stack_word_bytes": WORD[scene], "trace_form": "per_pixel", "primary_form": "none", "launched": 1})
    # 7. the service kernels, the device BIH build and the frames of the loop of sq_accumulate without groups
    add("camera_rays", "u16", "camera_rays", ["sq_camera_rays"], frame=FE)
    add("adaptive_update", "u16", "adaptive_update", ["sq_adaptive_update"], frame=FE)
    add("debug_tonemap", "u16", "debug_tonemap", ["sq_debug_kernel"])
    add("rng_fill", "u16", "rng_fill", ["sq_rng_fill", "sq_gen_bounce1<0>"], frame=F8, fresh=True)
    add("bih_build", "u16", "bih_build", ["k_init", "k_root", "k_centroid", "k_plane", "k_flag", "k_scan_sums", "k_scan_apply", "k_split",
                                          "k_scatter", "k_finish", "k_gather"])
    add("big_frame", "u16", "big", ["sq_accumulate<false, false>"], fresh=True)
    add("big_frame_masked", "u16", "big_masked", ["sq_accumulate<false, true>"], fresh=True)
    out.sort(key=lambda c: c.kind == "views")            # stable: a scene's multi-view cases after its others (module docstring)
    return out


CASES = _cases()
NAMES = [c.name for c in CASES]


# ---- running a case --------------------------------------------------------------------------------------------------------
class Walk:
    """The libraries, the two scenes on the host and (one per scene, reused) on the device, and the expected values, computed once."""

    def __init__(self):
        import torch
        O.lib()
        sqt.lib()
        self.torch = torch
        obj = open(os.path.join(SC.DATA, "scene.obj"), "rb").read()
        self.mesh = sqt.Mesh.from_text(obj, SC.BRIGHT_SQ)
        self.bih = sqt.BIH(self.mesh)
        self.ob = O.BIH(O.tris_from_text(obj, SC.BRIGHT_SQ))
        self.flat = self.ob.flatten()
        text = {"camera": open(os.path.join(SC.DATA, "camera"), "rb").read(), "rotated": SC.ROTATED}
        self.cam = {k: sqt.camera_from_text(v) for k, v in text.items()}
        self.ocam = {k: O.camera_from_text(v) for k, v in text.items()}
        self.restatement = Restatement(O, self.ob)
        self._scenes, self._ds = {}, {}
        self.device_error = []                                        # the first HIP error: after one, no case touches the device again

    @property
    def n_cu(self):
        return int(self.torch.cuda.get_device_properties(0).multi_processor_count)

    def scene(self, key):
        if key not in self._scenes:
            if key == "u16":
                self._scenes[key] = self.bih
            else:
                axis, side = SC.near_of(O, self.ocam["camera"])
                ps = SC.tall_u32(self.bih, U32_HEIGHT, axis, side)
                assert ps.height == U32_HEIGHT and ps.n_branches == 0x9000, (ps.height, ps.n_branches)
                self._scenes[key] = ps
        return self._scenes[key]

    def close(self):
        for ds in self._ds.values():
            ds.close()
        self._ds = {}

    # ---- expected values -----------------------------------------------------------------------------------------------------
    @functools.lru_cache(maxsize=None)
    def trails(self, cam, frame):
        w, h, spp = frame
        return SR.frame_paths(self.ob, self.flat, self.ocam[cam], spp, w, h)

    @functools.lru_cache(maxsize=None)
    def want_path_frame(self, cam, frame, depth, sky):
        """(sum, sum2, avg, rgb8) [w, h, 3] of the path-traced frame."""
        w, h, spp = frame
        s, q, avg = (a.reshape(w, h, 3) for a in SR.fold_frame(self.trails(cam, frame), depth, sky))
        rgb = tonemaps(O, avg)
        if depth == 3 and sky is None:                                # the oracle itself
            oavg, orgb, _ = self.ob.render(self.ocam[cam], spp, w, h, threads=RO.THREADS)
            assert same(avg, oavg) and np.array_equal(rgb, orgb), "sky_restatement differs from O.BIH.render"
            avg, rgb = oavg, orgb
        return s, q, avg, rgb

    @functools.lru_cache(maxsize=None)
    def want_cast_frame(self, cam, frame, n_lights):
        """(sum, sum2, avg, rgb8) [w, h, 3] of the cast frame under lights_of(n_lights), or the reference's light (None)."""
        w, h, spp = frame
        rays = [O.make_ray(w, h, y, x, self.ocam[cam]) for y in range(w) for x in range(h)]
        T, _ = self.restatement.radiance((cam, w, h), rays, lights_of(n_lights) if n_lights else [sqt.REFERENCE_LIGHT])
        s = fold_cast(T, 0, spp)
        with np.errstate(all="ignore"):
            q = fold_cast((T * T).astype(f32), 0, spp)
        avg = avg_of(s, spp).reshape(w, h, 3)
        rgb = tonemaps(O, avg)
        if not n_lights:
            oavg, orgb, _ = self.ob.render(self.ocam[cam], spp, w, h, cast=True, threads=RO.THREADS)
            assert same(avg, oavg) and np.array_equal(rgb, orgb), "lights_restatement differs from O.BIH.render"
            avg, rgb = oavg, orgb
        return s.reshape(w, h, 3), q.reshape(w, h, 3), avg, rgb

    def want_frame(self, c, cam="camera"):
        return self.want_cast_frame(cam, c.frame, c.lights) if c.cast else self.want_path_frame(cam, c.frame, c.depth, c.sky)

    @functools.lru_cache(maxsize=None)
    def rays(self, frame):
        """The camera rays of the frame and N_FREE_RAYS free rays, without -0 direction components (ray_oracle), with small, huge and
        negative seeds by thirds."""
        w, h, _ = frame
        cam_rays = [O.make_ray(w, h, y, x, self.ocam["camera"]) for y in range(w) for x in range(h)]
        rng = np.random.default_rng(w * 1000 + h)
        fo, fd = family_free(rng, self.bih.bounds, N_FREE_RAYS)
        o = np.ascontiguousarray(np.concatenate([np.array([r[0] for r in cam_rays], f32), fo]), f32)
        d = np.ascontiguousarray(positive_zeros(np.concatenate([np.array([r[1] for r in cam_rays], f32), fd])), f32)
        n = len(o)
        third = np.arange(n) % 3
        s = np.where(third == 0, rng.integers(0, 1 << 20, n), np.where(third == 1, rng.integers(1 << 40, 1 << 60, n), -rng.integers(1, 1 << 60, n)))
        return o, d, np.ascontiguousarray(s, np.int64)

    @functools.lru_cache(maxsize=None)
    def ray_trails(self, frame, k):
        o, d, s = self.rays(frame)
        return SR.paths(self.ob, self.flat, o, d, s, k=k)

    @functools.lru_cache(maxsize=None)
    def want_raytrace(self, frame, depth, sky):
        """(sum, avg, rgb8) per ray of the frame's ray batch at the frame's sample count."""
        spp = frame[2]
        rs = [SR.radiances(self.ray_trails(frame, k), depth, sky) for k in range(spp)]
        if depth == 3 and sky is None:
            o, d, s = self.rays(frame)
            for k in range(spp):
                assert same(from_zero(rs[k]), from_zero(oracle_raytrace(O, self.ob, o, d, s, k=k))), "sky_restatement differs from the oracle's raytrace"
        total = fold_list(rs)
        with np.errstate(all="ignore"):
            avg = ((f32(1) / f32(spp)) * total).astype(f32)
        return total, avg, tonemaps(O, avg)

    @functools.lru_cache(maxsize=None)
    def want_raycast(self, frame, n_lights):
        o, d, _ = self.rays(frame)
        T, _ = self.restatement.radiance(("batch",) + frame[:2], list(zip(o, d)), lights_of(n_lights) if n_lights else [sqt.REFERENCE_LIGHT])
        if not n_lights:                                              # the oracle's cast render is 1 * (0 + T); the query stores T
            assert same(from_zero(T), oracle_raycast(O, self.ob, o, d)), "lights_restatement differs from the oracle's raycast"
        return T

    @functools.lru_cache(maxsize=None)
    def want_hits(self, frame):
        o, d, _ = self.rays(frame)
        return oracle_hits(self.ob, o, d)

    # ---- the calls -----------------------------------------------------------------------------------------------------------
    def sync(self):
        self.torch.cuda.synchronize()

    def check_plan(self, ds, c):
        p = ds.last_plan()
        got = {k: p[k] for k in c.plan}
        assert got == c.plan, (c.name, "planned", got, "written for", c.plan)

    @staticmethod
    def live_mask(w, h):
        return np.add.outer(np.arange(w), np.arange(h)) % 2 == 0

    def run_render(self, ds, c):
        w, h, spp = c.frame
        avg, rgb = ds.render_rows(self.cam["camera"], spp, w, h, cast=c.cast)
        self.sync()
        self.check_plan(ds, c)
        _, _, want, want8 = self.want_frame(c)
        avg, rgb = avg.cpu().numpy(), rgb.cpu().numpy()
        assert same(avg, want), (c.name, "avg differs in pixels", int((canon(avg) != canon(want)).any(-1).sum()))
        assert np.array_equal(rgb, want8), (c.name, "rgb8")

    def check_masked(self, c, got, live, want, spp):
        s, q, avg, rgb = want
        dead = ~live
        assert same(got["sums"][live], s[live]), (c.name, "sum")
        assert same(got["sums2"][live], q[live]), (c.name, "sum2")
        assert (got["counts"][live] == spp).all(), (c.name, "count")
        assert same(got["avg"][live], avg[live]), (c.name, "avg")
        assert np.array_equal(got["rgb"][live], rgb[live]), (c.name, "rgb8")
        for k, v in MC.SENT.items():
            assert (got[k][dead] == v).all(), (c.name, "a dead pixel lost its sentinel", k)

    def run_masked(self, ds, c):
        w, h, spp = c.frame
        live = self.live_mask(w, h)
        B = MC.buffers(w, h)
        MC.masked(ds, self.cam["camera"], spp, w, h, 0, spp, B, live, cast=c.cast)
        self.check_plan(ds, c)
        self.check_masked(c, MC.host(B), live, self.want_frame(c), spp)

    def run_views(self, ds, c):
        w, h, spp = c.frame
        names = ("camera", "rotated")
        avg, rgb = ds.render_views([self.cam[n] for n in names], spp, w, h, cast=c.cast)
        self.sync()
        self.check_plan(ds, c)
        avg, rgb = avg.cpu().numpy(), rgb.cpu().numpy()
        for i, n in enumerate(names):
            _, _, want, want8 = self.want_frame(c, n)
            assert same(avg[i], want), (c.name, "view", n, "avg differs in pixels", int((canon(avg[i]) != canon(want)).any(-1).sum()))
            assert np.array_equal(rgb[i], want8), (c.name, "view", n, "rgb8")

    def run_raytrace(self, ds, c):
        o, d, s = self.rays(c.frame)
        r = ds.raytrace(o, d, seeds=s, samples=c.frame[2], want_rgb=True)
        self.sync()
        self.check_plan(ds, c)
        total, avg, rgb = self.want_raytrace(c.frame, c.depth, c.sky)
        assert same(r.sum.cpu().numpy(), total), (c.name, "sum differs in rays", int((canon(r.sum.cpu().numpy()) != canon(total)).any(-1).sum()))
        assert same(r.avg.cpu().numpy(), avg), (c.name, "avg")
        assert np.array_equal(r.rgb.cpu().numpy(), rgb), (c.name, "rgb8")

    def run_raycast(self, ds, c):
        o, d, _ = self.rays(c.frame)
        got = ds.raycast(o, d)
        self.sync()
        self.check_plan(ds, c)
        want = self.want_raycast(c.frame, c.lights)
        got = got.cpu().numpy()
        assert same(got, want), (c.name, "rays differ", int((canon(got) != canon(want)).any(-1).sum()))

    def run_intersect(self, ds, c):
        o, d, _ = self.rays(c.frame)
        got = ds.intersect(o, d)
        self.sync()
        self.check_plan(ds, c)
        check_hits(tuple(t.cpu().numpy() for t in got), self.want_hits(c.frame), c.name)

    def run_camera_rays(self, ds, c):
        w, h, _ = c.frame
        for name in ("camera", "rotated"):
            o, d = ds.camera_rays(self.cam[name], w, h)
            self.sync()
            want = [O.make_ray(w, h, y, x, self.ocam[name]) for y in range(w) for x in range(h)]
            assert same(o.cpu().numpy().reshape(-1, 3), np.array([r[0] for r in want], f32)), (c.name, name, "origins")
            assert same(d.cpu().numpy().reshape(-1, 3), np.array([r[1] for r in want], f32)), (c.name, name, "directions")

    def run_adaptive_update(self, ds, c):
        """The stopping rule on the moments of the frame's restatement after 2 and 3 samples, and on rows that sit on its edges."""
        torch = self.torch
        w, h, spp = c.frame
        trails = self.trails("camera", c.frame)
        for n in (2, spp):
            s, q, _ = (a.reshape(w, h, 3) for a in SR.fold_frame(trails[:n], 3, None))
            counts = np.full((w, h), n, np.int32)
            counts[0, ::7] = 1                                          # fewer than two samples: never converged
            mask = np.ones((w, h), np.uint8)
            mask[1, ::5] = 0                                            # already stopped: stays stopped
            for tol, eps in ((0.5, 1.0), (0.05, 0.0), (0.0, 1.0)):
                dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (s, q, counts, mask)]
                live = ds.adaptive_update(dev[0], dev[1], dev[2], dev[3], tol, eps)
                want = sqt.rule_reference(s, q, counts, mask, tol, eps)
                got = dev[3].cpu().numpy()
                assert np.array_equal(got, want), (c.name, n, tol, eps, int((got != want).sum()))
                assert live == int(want.sum()), (c.name, n, tol, eps, live)

    def run_debug_tonemap(self, ds, c):
        rng = np.random.default_rng(8)
        rows = np.concatenate([rng.uniform(0, 2, (DEBUG_ROWS - 6, 3)), [[0, 0, 0], [1, 1, 1], [-0.0, 0.5, 2.0], [-1, np.nan, 3e38], [np.inf, -np.inf, 0.25],
                                                                         [-3e38, 1e-30, -1e-30]]]).astype(f32)
        got = sqt._native.debug_eval("tonemap", rows)
        assert np.array_equal(got, tonemaps(O, rows)), c.name

    def run_rng_fill(self, ds, c):
        """The first frame of a fresh scene fills its table of generator words: the frame is the oracle's, the entries are O.tfgen_words'."""
        assert ds.rng_table()[0] == 0
        RO.set_sky_options(ds)
        w, h, spp = c.frame
        avg, rgb = ds.render_rows(self.cam["camera"], spp, w, h)
        self.sync()
        _, _, want, want8 = self.want_path_frame("camera", c.frame, 3, None)
        assert same(avg.cpu().numpy(), want) and np.array_equal(rgb.cpu().numpy(), want8), c.name
        cover = ds.rng_table()[0]
        assert cover >= w * h * spp, cover
        n = min(cover, 4096)
        for first in (0, cover - n):
            got = ds.rng_table(first, n)[1]
            want_words = np.array([O.tfgen_words(first + i)[:3] for i in range(n)], np.uint32)
            assert np.array_equal(got, want_words), (c.name, first)

    def run_bih_build(self, ds, c):
        raw = lambda a: np.ascontiguousarray(a).view(np.uint8)  # noqa: E731
        host, dev = self.bih, sqt.BIH(self.mesh, device=0)
        assert host.scene.n_tris > 2048                                 # more than one block of the scan
        assert (dev.height, dev.num_leaves, dev.longest_leaf) == (host.height, host.num_leaves, host.longest_leaf)
        assert dev.scene.n_nodes == host.scene.n_nodes and dev.scene.n_tris == host.scene.n_tris
        for name in ("bounds", "nodes", "tris", "materials"):
            assert np.array_equal(raw(getattr(dev, name)), raw(getattr(host, name))), (c.name, name)

    def big_frame(self):
        """(rows, columns, the oracle's one-sample frame): more pixels than n_cu x 256 threads, so that with aux_blocks_per_cu = 1 the
        loop of sq_accumulate without groups runs."""
        w, h = self.n_cu + 1, BIG_COLUMNS
        assert w * h > self.n_cu * 256, (w, h, self.n_cu)
        if not hasattr(self, "_big"):
            self._big = self.ob.render(self.ocam["camera"], 1, w, h, threads=RO.THREADS)[:2]
        return w, h, self._big

    def run_big(self, ds, c):
        w, h, (want, want8) = self.big_frame()
        RO.set_sky_options(ds)
        ds.set_option("aux_blocks_per_cu", 1)
        avg, rgb = ds.render_rows(self.cam["camera"], 1, w, h)
        self.sync()
        p = ds.last_plan()
        assert (p["variant"], p["stack_word_bytes"], p["trace_form"], p["primary_form"], p["launched"]) == (2, 2, "resident", "resident", 1), p
        assert same(avg.cpu().numpy(), want) and np.array_equal(rgb.cpu().numpy(), want8), c.name

    def run_big_masked(self, ds, c):
        """One sample: sum = 0 + r = avg, and sum2 = 0 + r * r = sum * sum, also where r is -0 (both squares are +0)."""
        w, h, (want, want8) = self.big_frame()
        RO.set_sky_options(ds)
        ds.set_option("aux_blocks_per_cu", 1)
        live = self.live_mask(w, h)
        B = MC.buffers(w, h)
        MC.masked(ds, self.cam["camera"], 1, w, h, 0, 1, B, live)
        p = ds.last_plan()
        assert (p["variant"], p["stack_word_bytes"], p["trace_form"], p["primary_form"], p["launched"]) == (2, 2, "resident", "resident", 1), p
        with np.errstate(all="ignore"):
            q = (want * want).astype(f32)
        self.check_masked(c, MC.host(B), live, (want, q, want, want8), 1)

    def run(self, index):
        """Case `index`, behind its marker: a one-element debug_eval of the index (the oracle's generator words of it come back)."""
        c = CASES[index]
        if self.device_error:
            raise RuntimeError(f"not run: the device reported an error earlier in this process ({self.device_error[0]})")
        ds = None
        try:
            words = sqt._native.debug_eval("tfgen3", [index])
            assert [int(v) for v in words[0]] == O.tfgen_words(index)[:3], "marker"
            if c.fresh:
                ds = sqt.DeviceScene(self.scene(c.scene), 0)
            else:
                if c.scene not in self._ds:
                    self._ds[c.scene] = sqt.DeviceScene(self.scene(c.scene), 0)
                ds = self._ds[c.scene]
                RO.set_sky_options(ds, sky=c.sky, depth=c.depth, **c.opts)
                ds.set_option("cast_wavefront", c.cast_wavefront)
                if c.lights:
                    ds.set_lights(lights_of(c.lights))
            getattr(self, "run_" + c.kind)(ds, c)
        except sqt.SquiglyError as e:
            if " failed: " in str(e):                                   # a HIP error: nothing more runs on this device
                self.device_error.append(f"{c.name}: {e}")
            raise
        except RuntimeError as e:                                       # torch's own report of a HIP error (a synchronize, a copy)
            if "HIP error" in str(e) or "CUDA error" in str(e):
                self.device_error.append(f"{c.name}: {e}")
            raise
        finally:
            if ds is not None and not self.device_error:
                if c.fresh:
                    ds.close()
                else:                                                   # the option tables and the scene state, as every case finds them
                    RO.set_sky_options(ds)
                    if c.lights:
                        ds.set_lights(None)


def main(out_path):
    walk = Walk()
    results = {}
    try:
        for i, c in enumerate(CASES):
            try:
                walk.run(i)
                results[c.name] = "passed"
            except Exception as e:  # noqa: BLE001
                results[c.name] = f"{type(e).__name__}: {e}"[:500]
            print(i, c.name, results[c.name], flush=True)
        walk.sync() if not walk.device_error else None
    finally:
        if not walk.device_error:
            walk.close()
    with open(out_path, "w") as f:
        json.dump({"build_id": sqt._native.build_id(), "cases": NAMES, "results": results, "n_cu": walk.n_cu}, f, indent=1)
    return 0 if all(v == "passed" for v in results.values()) else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
