#!/usr/bin/env python3
"""Records what the library plans for a list of tiny calls, through the public Python API alone, into tests/golden/plan_cases.json:

    SQ_LIB_PATH=<library of the commit to record> python tools/record_plans.py --commit <its hash> [--out FILE]

Needs a GPU.  Run it against the commit whose planning is the yardstick (tests/test_plan.py holds sq_plan_call to the file), never
against the code under test.  Per case the file holds the inputs (scene, options, depth, sky, lights, call), the 14 fields of
sq_plan as DeviceScene.last_plan() gives them (null when the call was refused before it planned), the number of launches option
"timing" bracketed (the trace kernel's, or the one per-lane kernel's) and the refusal's text (null when the call went through).
Every case runs on a DeviceScene of its own, so the workspace holds exactly the slots the call asked for.

cases() and scene_of() are what tests/test_plan.py imports: the same list, and the same scenes packed on the CPU.
"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
DATA = os.path.join(ROOT, "data")
OUT = os.path.join(ROOT, "tests", "golden", "plan_cases.json")
PLAN_FIELDS = ["launched", "variant", "stack_word_bytes", "height", "stack_cap", "trace_form", "blocks_per_cu", "n_lds",
               "trace_lds_bytes", "pixel_lds_bytes", "primary_form", "packed_leaves", "n_emitters", "level1_cull"]
SKY = ((0.5, 0.6, 0.7), (0.1, 0.1, 0.1))
AXIS, SIDE = 0, 0          # the padding's orientation (tree_padding.LEFT): a plan depends on the padded tree's size alone


def lights_of(n):
    return [((0.1 * i, 3.0, -1.0), (2.0, 1.0 + 0.25 * i, 2.0)) for i in range(n)]


def cases():
    """The list of cases: dicts of name, scene, options, depth, sky, lights and call.  Frames are w rows x h columns."""
    out = []

    def add(name, call, opts=None, scene=None, depth=None, sky=False, lights=None):
        assert all(c["name"] != name for c in out), name
        out.append({"name": name, "scene": scene or {"kind": "obj"}, "options": opts or {}, "depth": depth, "sky": sky,
                    "lights": lights, "call": call})

    def frame(w, h, samples, cast=False, kind="render", **kw):
        return dict({"kind": kind, "w": w, "h": h, "samples": samples, "cast": cast}, **kw)
    f1, f8, f370 = frame(1, 1, 1), frame(8, 8, 2), frame(3, 70, 3)
    # data/scene.obj: the resident form and every option that chooses a form
    add("default_8x8", f8)
    add("default_1x1", f1)
    add("default_3x70", f370)
    add("variant1_8x8", f8, {"variant": 1})
    add("variant1_3x70", f370, {"variant": 1})
    add("pool0", f8, {"pool": 0})
    add("profile1", f8, {"profile": 1})
    add("profile1_pool0", f8, {"profile": 1, "pool": 0})
    add("primary_resident0", f8, {"primary_resident": 0})
    add("primary_pooled1", f8, {"primary_pooled": 1})
    add("primary_pooled1_pool0", f8, {"primary_pooled": 1, "pool": 0})
    add("primary_tiles0_per_lane_3x70", f370, {"primary_tiles": 0, "primary_resident": 0})
    add("level1_cull0", f8, {"level1_cull": 0})
    add("cull0", f8, {"cull": 0})
    add("resident0", f8, {"resident": 0})
    add("resident0_pool0", f8, {"resident": 0, "pool": 0})
    add("resident0_profile1", f8, {"resident": 0, "profile": 1})
    add("resident0_primary_pooled1", f8, {"resident": 0, "primary_pooled": 1})
    for per_cu in (1, 2, 3, 8):
        add(f"resident0_blocks{per_cu}", f8, {"resident": 0, "trace_blocks_per_cu": per_cu})
    for kb in (0, 128):
        for per_cu in (0, 2):
            add(f"resident0_kb{kb}_blocks{per_cu}", f8, {"resident": 0, "lds_node_kb": kb, "trace_blocks_per_cu": per_cu})
    # batches: `slots` at the pixel count gives one sample of every pixel per batch
    add("batches_8x8_5spp", frame(8, 8, 5), {"slots": 64})
    add("batches_3x70_3spp", f370, {"slots": 210})
    add("batches_slots1", frame(8, 8, 3), {"slots": 1})
    add("batches_two_per_batch", frame(8, 8, 5), {"slots": 128})
    add("range_1_3_of_5", frame(8, 8, 5, kind="range", k_begin=1, k_end=3), {"slots": 64})
    # the overlapped schedules: two tracks of one sample per pixel
    for ov in (1, 2):
        for spp in (1, 3, 4):
            add(f"overlap{ov}_{spp}spp", frame(8, 8, spp), {"overlap": ov, "slots": 128})
        add(f"overlap{ov}_one_track_of_slots", frame(8, 8, 3), {"overlap": ov, "slots": 64})
        add(f"overlap{ov}_primary_pooled", frame(8, 8, 3), {"overlap": ov, "slots": 128, "primary_pooled": 1})
        add(f"overlap{ov}_resident0", frame(8, 8, 3), {"overlap": ov, "slots": 128, "resident": 0})
    add("overlap1_polite", frame(8, 8, 4), {"overlap": 1, "slots": 128, "aux_polite": 2})
    add("overlap1_deep_falls_back", frame(8, 8, 3), {"overlap": 1, "slots": 128}, depth=4)
    # cast frames
    cast8 = frame(8, 8, 1, cast=True)
    add("cast", cast8)
    add("cast_lights3", cast8, lights=3)
    add("cast_variant1_lights3", cast8, {"variant": 1}, lights=3)
    add("cast_wavefront_reference_light", cast8, {"cast_wavefront": 1})
    add("cast_wavefront_1_light", cast8, {"cast_wavefront": 1}, lights=1)
    add("cast_wavefront_5_lights_1_per_batch", cast8, {"cast_wavefront": 1, "slots": 64}, lights=5)
    add("cast_wavefront_5_lights_2_per_batch", cast8, {"cast_wavefront": 1, "slots": 128}, lights=5)
    add("cast_wavefront_5_lights_one_batch", cast8, {"cast_wavefront": 1}, lights=5)
    add("cast_wavefront_variant1", cast8, {"cast_wavefront": 1, "variant": 1}, lights=2)
    add("cast_wavefront_resident0", frame(3, 70, 1, cast=True), {"cast_wavefront": 1, "resident": 0, "slots": 210}, lights=3)
    # path depth and sky
    for depth in (1, 2, 3, 4, 8):
        for sky in (False, True):
            add(f"depth{depth}{'_sky' if sky else ''}", f8, depth=depth, sky=sky)
    for depth in (1, 3, 4):
        for sky in (False, True):
            add(f"variant1_depth{depth}{'_sky' if sky else ''}", f8, {"variant": 1}, depth=depth, sky=sky)
    add("deep_option_depth3", f8, {"deep": 1})
    add("depth4_batches", frame(8, 8, 3), {"slots": 64}, depth=4)
    add("depth8_sky_batches", frame(3, 70, 3), {"slots": 210}, depth=8, sky=True)
    add("depth2_primary_pooled", f8, {"primary_pooled": 1}, depth=2)
    add("depth5_resident0", f8, {"resident": 0}, depth=5)
    add("cast_ignores_depth_and_sky", cast8, depth=5, sky=True)
    # masked calls, views
    add("masked_mom2", frame(8, 8, 2, kind="masked", mom2=True))
    add("masked_mom2_batches", frame(8, 8, 3, kind="masked", mom2=True), {"slots": 64})
    add("masked_no_mom2", frame(8, 8, 2, kind="masked", mom2=False))
    add("masked_mom2_variant1", frame(8, 8, 2, kind="masked", mom2=True), {"variant": 1})
    add("masked_mom2_depth4_sky", frame(8, 8, 2, kind="masked", mom2=True), depth=4, sky=True)
    add("masked_mom2_cast_lights", frame(8, 8, 1, cast=True, kind="masked", mom2=True), lights=2)
    add("views2", frame(8, 8, 2, kind="views", n_views=2))
    add("views2_variant1", frame(8, 8, 2, kind="views", n_views=2), {"variant": 1})
    add("views2_3x70_batches", frame(3, 70, 3, kind="views", n_views=2), {"slots": 420})
    add("views2_depth4_sky", frame(8, 8, 2, kind="views", n_views=2), depth=4, sky=True)
    add("views2_cast_wavefront", frame(8, 8, 1, cast=True, kind="views", n_views=2), {"cast_wavefront": 1}, lights=3)
    add("views3_per_lane_primary", frame(3, 70, 2, kind="views", n_views=3), {"primary_resident": 0})
    # queries (rays: the camera rays of a w x h frame)
    isect = frame(8, 8, 1, kind="intersect")
    add("intersect", isect)
    add("intersect_variant1", isect, {"variant": 1})
    add("intersect_chunks", frame(3, 70, 1, kind="intersect"), {"slots": 64})
    add("intersect_resident0", isect, {"resident": 0})
    add("intersect_pool0_profile1", isect, {"pool": 0, "profile": 1})
    rt = frame(8, 8, 2, kind="raytrace")
    add("raytrace", rt)
    add("raytrace_variant1", rt, {"variant": 1})
    add("raytrace_chunks", frame(3, 70, 2, kind="raytrace"), {"slots": 64})
    add("raytrace_depth4_sky", rt, depth=4, sky=True)
    add("raytrace_variant1_depth2", rt, {"variant": 1}, depth=2)
    add("raytrace_primary_pooled", rt, {"primary_pooled": 1})
    add("raytrace_resident0_batches", frame(8, 8, 3, kind="raytrace"), {"resident": 0, "slots": 64})
    rc = frame(8, 8, 1, kind="raycast")
    add("raycast", rc)
    add("raycast_lights3", rc, lights=3)
    add("raycast_wavefront_lights3", rc, {"cast_wavefront": 1, "slots": 64}, lights=3)
    add("raycast_variant1", rc, {"variant": 1})
    # a streaming scene: the height field of tools/gen_scenes.py with more than 4096 vertices
    hf = {"kind": "heightfield", "n": 64}
    add("hf", f8, scene=hf)
    add("hf_variant1", f8, {"variant": 1}, scene=hf)
    add("hf_pool0", f8, {"pool": 0}, scene=hf)
    add("hf_profile1", f8, {"profile": 1}, scene=hf)
    add("hf_primary_pooled1", f8, {"primary_pooled": 1}, scene=hf)
    for per_cu in (1, 2, 3):
        add(f"hf_blocks{per_cu}", f8, {"trace_blocks_per_cu": per_cu}, scene=hf)
    for kb in (0, 1, 128):
        add(f"hf_kb{kb}", f8, {"lds_node_kb": kb}, scene=hf)
        add(f"hf_kb{kb}_blocks2", f8, {"lds_node_kb": kb, "trace_blocks_per_cu": 2}, scene=hf)
    add("hf_depth4_sky", f8, scene=hf, depth=4, sky=True)
    add("hf_intersect", isect, scene=hf)
    add("hf_overlap2", frame(8, 8, 3), {"overlap": 2, "slots": 128}, scene=hf)
    add("hf_cast_wavefront", cast8, {"cast_wavefront": 1}, scene=hf, lights=2)
    # data/scene.obj padded to the heights on both sides of every form change (tests/test_gpu_limits.py, EXPECT), 2-byte stack words ...
    for h in (14, 46, 47, 158, 159):
        add(f"u16_height{h}", f1, scene={"kind": "padded", "height": h})
    for h in (14, 15, 159, 160):
        add(f"u16_height{h}_pool0", f1, {"pool": 0}, scene={"kind": "padded", "height": h})
    for h in (46, 47):
        add(f"u16_height{h}_8x8", f8, scene={"kind": "padded", "height": h})
    for h in (320, 321):
        add(f"u16_height{h}_variant1", f1, {"variant": 1}, scene={"kind": "padded", "height": h})
    add("u16_height159_intersect", isect, scene={"kind": "padded", "height": 159})
    add("u16_height321_intersect_variant1", isect, {"variant": 1}, scene={"kind": "padded", "height": 321})
    add("u16_height321_cast", frame(1, 1, 1, cast=True), scene={"kind": "padded", "height": 321})
    add("u16_height159_raytrace", frame(1, 1, 1, kind="raytrace"), scene={"kind": "padded", "height": 159})
    # ... and 4-byte ones (0x9000 branches)
    for h in (23, 24, 79, 80):
        add(f"u32_height{h}", f1, scene={"kind": "padded_u32", "height": h})
    for h in (160, 161):
        add(f"u32_height{h}_variant1", f1, {"variant": 1}, scene={"kind": "padded_u32", "height": h})
    add("u32_height24_8x8_depth4", f8, scene={"kind": "padded_u32", "height": 24}, depth=4)
    # frames too large for one call: refused before the device is touched
    add("refuse_2_29_pixels", frame(16385, 32768, 1))
    add("refuse_2_31_pixels_variant1", frame(46341, 46341, 1), {"variant": 1})
    add("refuse_2_31_pixels_cast", frame(65536, 32768, 1, cast=True))
    add("refuse_views_2_29_pixels", frame(16385, 16384, 1, kind="views", n_views=2))
    add("refuse_2_32_tile_lanes", frame(1 << 26, 1, 1, kind="render_no_buffer"), {"primary_resident": 0, "primary_tiles": 0})
    return out


_scene_cache = {}


def scene_of(sqt, spec):
    """The scene of a case's `scene` entry: an object with .scene (an sq_scene), kept for the process."""
    import tree_padding as TP
    key = json.dumps(spec, sort_keys=True)
    if key in _scene_cache:
        return _scene_cache[key]
    if spec["kind"] == "heightfield":
        import gen_scenes
        obj, sq, _ = gen_scenes.heightfield_scene(spec["n"])
        s = sqt.BIH(sqt.Mesh.from_text(obj, sq))
    else:
        base = scene_of(sqt, {"kind": "obj"}) if spec["kind"] != "obj" else sqt.BIH(sqt.Mesh.from_obj(os.path.join(DATA, "scene.obj"), DATA))
        if spec["kind"] == "obj":
            s = base
        elif spec["kind"] == "padded":
            s = TP.full_stack(base, spec["height"], AXIS, SIDE)
        else:                                     # padded_u32: tests/test_gpu_limits.py, _tall_u32
            nb0 = int(((base.nodes["kind"] & 3) != 3).sum())
            inner = TP.full_stack_wrappers(base, spec["height"] - 1, AXIS, SIDE)
            s = TP.PaddedScene(base, {0: [(AXIS, SIDE, ("balanced", 0x9000 - nb0 - len(inner) - 12 - 1))] + inner})
        if spec["kind"] != "obj":
            assert s.height == spec["height"], (spec, s.height)
    _scene_cache[key] = s
    return s


def run_case(sqt, case, cam):
    import torch
    ds = sqt.DeviceScene(scene_of(sqt, case["scene"]), 0)
    refusal = None
    try:
        ds.set_option("timing", 1)
        for k, v in case["options"].items():
            ds.set_option(k, v)
        if case["depth"] is not None:
            ds.set_depth(case["depth"])
        if case["sky"]:
            ds.set_sky(*SKY)
        if case["lights"] is not None:
            ds.set_lights(lights_of(case["lights"]))
        ds.reset_timing()
        c = case["call"]
        w, h, n, cast, kind = c["w"], c["h"], c["samples"], c["cast"], c["kind"]
        dev = torch.device("cuda", 0)
        try:
            if kind == "render":
                ds.render_rows(cam, n, w, h, cast=cast)
            elif kind == "render_no_buffer":      # a refusal is expected: nothing is written
                ds.render_rows(cam, n, w, h, cast=cast, want_avg=False, out_rgb=torch.zeros(16, dtype=torch.uint8, device=dev))
            elif kind == "range":
                ds.render_rows_range(cam, n, w, h, c["k_begin"], c["k_end"], torch.zeros((w, h, 3), dtype=torch.float32, device=dev), cast=cast)
            elif kind == "masked":
                mask = torch.ones((w, h), dtype=torch.uint8, device=dev)
                mask[0, 0] = 0
                ds.render_rows_masked(cam, n, w, h, 0, n, torch.zeros((w, h, 3), dtype=torch.float32, device=dev), mask=mask,
                                      sums2=torch.zeros((w, h, 3), dtype=torch.float32, device=dev) if c["mom2"] else None,
                                      counts=torch.zeros((w, h), dtype=torch.int32, device=dev), cast=cast)
            elif kind == "views":
                ds.render_views([cam] * c["n_views"], n, w, h, cast=cast)
            else:
                o, d = ds.camera_rays(cam, w, h)
                o, d = o.reshape(-1, 3), d.reshape(-1, 3)
                if kind == "intersect":
                    ds.intersect(o, d)
                elif kind == "raytrace":
                    ds.raytrace(o, d, samples=n)
                else:
                    assert kind == "raycast", kind
                    ds.raycast(o, d)
            torch.cuda.synchronize()
        except sqt.SquiglyError as e:
            refusal = str(e)
        try:
            plan = ds.last_plan()
        except sqt.SquiglyError:
            plan = None                           # refused before the call planned anything
        launches = ds.kernel_timing()[1]
    finally:
        ds.close()
    return {"plan": plan, "trace_launches": int(launches), "refusal": refusal}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--commit", required=True, help="the commit the loaded library was built from")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    import torch
    sqt = importlib.import_module("squigly-trace_amd")
    cam = sqt.load_camera(os.path.join(DATA, "camera"))
    n_cu = int(torch.cuda.get_device_properties(0).multi_processor_count)
    rows = []
    for case in cases():
        rows.append(dict(case, **run_case(sqt, case, cam)))
        print(case["name"], rows[-1]["plan"] and rows[-1]["plan"]["trace_form"], rows[-1]["trace_launches"], rows[-1]["refusal"], flush=True)
    head = {"commit": args.commit, "library": sqt._native.build_id(),
            "how": "tools/record_plans.py on an MI355X with SQ_LIB_PATH at that commit's library: DeviceScene.last_plan(), "
                   "kernel_timing() under option timing, and the refusal's text, one DeviceScene per case",
            "n_cu": n_cu, "plan_fields": PLAN_FIELDS}
    with open(args.out, "w") as f:
        f.write("{\n" + ",\n".join(f' "{k}": {json.dumps(v)}' for k, v in head.items()) + ',\n "cases": [\n')
        f.write(",\n".join("  " + json.dumps(r) for r in rows))
        f.write("\n ]\n}\n")
    print(f"{len(rows)} cases -> {args.out}")


if __name__ == "__main__":
    main()
