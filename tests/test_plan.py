"""The call planner (csrc/sq_plan.h, sq_host.cpp: plan_call, plan_schedule, workspace_layout) through its C-ABI window sq_plan_call
(include/squigly_host.h), on the CPU.

* the plan is the parent's plan: tests/golden/plan_cases.json holds, for every case of tools/record_plans.py, what the commit before
  the planner was lifted out of sq_device.hip planned on an MI355X -- the 14 fields of sq_plan, the launches option "timing" counted
  and the refusal's text (the JSON says which commit and how).  Every case is packed on the CPU and planned through the window;
* structure, independent of that commit: workspace offsets, batch arithmetic, reservation sizes;
* the option table: every range refusal with its exact text.
"""
import ctypes as C
import json
import os
import sys

import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_plans as R  # noqa: E402

GOLD = json.load(open(os.path.join(GOLDEN, "plan_cases.json")))
CASES = {c["name"]: c for c in GOLD["cases"]}
PACKED = ["n_branches", "n_verts", "height", "small_index", "packed_leaves", "n_emitters", "nonneg_materials", "finite_geometry",
          "shortcut_depth", "level1_on"]
OUT = ["path", "ad", "mom2", "sky", "deep", "pixels", "px_blocks", "px_lds", "n_call", "slots", "trace_form", "resident", "pool", "profile", "dense",
       "n_lds", "stack_cap", "trace_blocks", "trace_threads", "tr_lds", "primary_grid", "primary_lds", "aux_blocks", "acc_grouped",
       "level1_cull", "deep_slot_bytes", "need_lights", "need_sum2", "need_deep", "rng_table", "rng_grow", "chunk_rays", "have_slots",
       "overlap", "tracks", "track_slots", "batch", "n_batches", "n_real", "query_chunk", "tail_kc", "pp_grid_x", "pp_grid_y",
       "tail_pp_grid_x", "tail_pp_grid_y", "chunk_0", "chunk_1", "guide_shift_0", "guide_shift_1", "pixel_major", "tail_chunk",
       "lone_chunk", "deep_oxy", "deep_trail", "deep_tmiss"]
WS = ["ws_cnt", "ws_stats", "ws_pix", "ws_t0", "ws_tri0", "ws_sum", "ws_mt", "ws_mtri", "ws_state", "ws_org", "ws_dir", "ws_tri1", "ws_carry",
      "ws_total"]
LANE_CAST, LANE_DEEP, LANE_PLAIN, WAVE_CAST, WAVE_DEEP, PIPELINE, QUERY_LANES, QUERY_WAVE = range(8)


def plan_call(sqt, inputs, have_slots=0, outputs=OUT + WS):
    """sq_plan_call: (return code, plan dict as DeviceScene.last_plan gives it, {scalar: value}, sq_last_error's text)."""
    N, L = sqt._native, sqt.lib()
    names = (C.c_char_p * len(inputs))(*[k.encode() for k in inputs])
    values = (C.c_int64 * len(inputs))(*[int(v) for v in inputs.values()])
    onames = (C.c_char_p * len(outputs))(*[k.encode() for k in outputs])
    ovalues = (C.c_int64 * len(outputs))()
    p = N.Plan()
    rc = L.sq_plan_call(names, values, len(inputs), have_slots, C.byref(p), onames, ovalues, len(outputs))
    plan = {name: int(getattr(p, name)) for name, _ in N.Plan._fields_}
    plan["trace_form"], plan["primary_form"] = N.TRACE_FORMS[plan["trace_form"]], N.PRIMARY_FORMS[plan["primary_form"]]
    return rc, plan, dict(zip(outputs, [int(v) for v in ovalues])), L.sq_last_error().decode()


_scalars = {}


def scene_scalars(sqt, spec):
    """The planner's scene inputs of a case's scene, from the packer (sq_scene_pack) on the CPU."""
    key = json.dumps(spec, sort_keys=True)
    if key not in _scalars:
        holder, L, h = R.scene_of(sqt, spec), sqt.lib(), C.c_void_p()
        sqt._native.check(L.sq_scene_pack(C.byref(holder.scene), C.byref(h)))
        try:
            out = {}
            for name in PACKED:
                v = C.c_int64()
                assert L.sq_packed_scalar(h, name.encode(), C.byref(v)) == 0, name
                out[name] = v.value
            data, n = C.c_void_p(), C.c_size_t()
            assert L.sq_packed_array(h, b"trix", C.byref(data), C.byref(n)) == 0
            out["trix"], out["n_tris"] = int(n.value > 0), holder.scene.n_tris
        finally:
            L.sq_packed_free(h)
        _scalars[key] = out
    return _scalars[key]


def case_inputs(sqt, case):
    """(the named inputs of the case's call, the rays of a query or None): what render_rows and the query entry points make of it."""
    c, opts = case["call"], case["options"]
    inp = dict(scene_scalars(sqt, case["scene"]), n_cu=GOLD["n_cu"], **opts)
    inp.update(depth=case["depth"] or 3, sky=int(case["sky"]), lights_set=int(case["lights"] is not None), n_lights=case["lights"] or 1)
    kind, w, h, n = c["kind"], c["w"], c["h"], c["samples"]
    if kind == "intersect":
        inp.update(query=1, n_rays=w * h)
        return inp, None
    if kind in ("raytrace", "raycast"):            # chunk by chunk a frame of one row (radiance_rays); h comes with the chunk
        inp.update(source=2, cast=int(kind == "raycast"), local_rows=1, tile_rows=1, k_begin=0, k_end=n if kind == "raytrace" else 1, total_rays=w * h)
        return inp, w * h
    tile_rows = 8 if opts.get("primary_tiles", 1) else 1      # a whole image in one shard (render_rows)
    inp.update(source=int(kind == "views"), cast=int(c["cast"]), masked=int(kind == "masked"), mom2=int(c.get("mom2", False)),
               n_views=c.get("n_views", 1), local_rows=w, h=h, tile_rows=tile_rows, tiles_x=-(-h // (64 // tile_rows)),
               k_begin=c.get("k_begin", 0), k_end=c.get("k_end", n))
    return inp, None


def launches_of(plan, v, depth, n_rays=None):
    """The launches option "timing" brackets, as the schedule implies them: the one per-lane kernel, or the trace kernel's."""
    pooled, path = int(plan["primary_form"] == "pooled"), v["path"]
    if path in (LANE_CAST, LANE_DEEP, LANE_PLAIN):
        return 1
    if path == QUERY_LANES:
        return -(-n_rays // 2 ** 30)
    if path == QUERY_WAVE:
        return -(-n_rays // v["query_chunk"])
    if path == WAVE_CAST:
        return v["n_real"] + pooled
    if path == WAVE_DEEP:
        return v["n_real"] * (depth - 1) + pooled
    return 2 * v["n_real"] + pooled + v["overlap"]            # the overlapped schedules give the mirror rays a launch of their own


def check_structure(v):
    """What holds for every planned wavefront call, whatever was recorded."""
    offs = [v[k] for k in WS]
    assert all(a < b for a, b in zip(offs, offs[1:])) and all(o % 256 == 0 for o in offs), offs
    if v["path"] in (WAVE_CAST, WAVE_DEEP, PIPELINE):
        assert 1 <= v["n_real"] <= v["n_batches"] and v["batch"] * v["n_batches"] >= v["n_call"] >= 1, v
        assert v["batch"] * v["pixels"] <= v["track_slots"] and v["tracks"] * v["track_slots"] <= v["have_slots"], v
        assert v["tracks"] == 1 + v["overlap"] and (v["n_real"] - 1) * v["batch"] + v["tail_kc"] == v["n_call"], v
        assert 1 <= v["pp_grid_x"] and 1 <= v["pp_grid_y"] <= 64, v
    cap = 512 if v["resident"] else 128
    for k in ("chunk_0", "chunk_1", "tail_chunk", "lone_chunk"):
        assert v[k] % 64 == 0 and 64 <= v[k] <= cap, (k, v)


def run_case(sqt, case):
    """(plan, launches, refusal) of a case through the planner: a radiance query chunk by chunk, as radiance_rays plans it."""
    inp, rays = case_inputs(sqt, case)
    depth = case["depth"] or 3
    if rays is None:
        rc, plan, v, err = plan_call(sqt, inp)
        assert rc in (0, 1), err
        if rc:
            return plan, 0, err
        if v["slots"]:
            check_structure(v)
        return plan, launches_of(plan, v, depth, inp.get("n_rays")), None
    rc, plan, v, err = plan_call(sqt, dict(inp, h=rays, tiles_x=-(-rays // 64)), outputs=["chunk_rays"])
    chunk = v["chunk_rays"] if rc == 0 else rays   # a refusal comes from the first chunk, the largest
    launches = 0
    for c0 in range(0, rays, chunk):
        m = min(chunk, rays - c0)
        rc, plan, v, err = plan_call(sqt, dict(inp, h=m, tiles_x=-(-m // 64)))
        assert rc in (0, 1), err
        if rc:
            return plan, launches, err
        if v["slots"]:
            check_structure(v)
        launches += launches_of(plan, v, depth)
    return plan, launches, None


def test_the_recording_is_the_parents():
    assert GOLD["commit"].startswith("d51a3a3") and GOLD["plan_fields"] == R.PLAN_FIELDS
    assert [c["name"] for c in GOLD["cases"]] == [c["name"] for c in R.cases()]
    for rec, case in zip(GOLD["cases"], R.cases()):
        assert {k: rec[k] for k in case} == case, case["name"]


def test_the_cases_cover_every_form_and_schedule():
    """What tools/record_plans.py promises of its list, asserted on what was recorded."""
    planned = [c for c in GOLD["cases"] if c["plan"]]
    have = lambda f: {f(c) for c in planned}                   # noqa: E731
    assert have(lambda c: c["plan"]["trace_form"]) == {"per_pixel", "resident", "streaming_six_wave", "streaming_plain"}
    assert have(lambda c: c["plan"]["primary_form"]) == {"none", "per_lane", "resident", "pooled"}
    assert have(lambda c: c["plan"]["stack_word_bytes"]) == {2, 4} and have(lambda c: c["plan"]["variant"]) == {1, 2}
    assert have(lambda c: c["plan"]["blocks_per_cu"]) >= {0, 1, 2, 3} and have(lambda c: c["plan"]["level1_cull"]) == {0, 1}
    opt = lambda c, k, d: c["options"].get(k, d)              # noqa: E731
    assert have(lambda c: opt(c, "pool", 1)) == {0, 1} and 1 in have(lambda c: opt(c, "profile", 0))
    assert have(lambda c: opt(c, "trace_blocks_per_cu", 0)) >= {0, 1, 2, 3} and have(lambda c: opt(c, "lds_node_kb", 32)) >= {0, 128}
    assert have(lambda c: opt(c, "level1_cull", 1)) == {0, 1}
    for ov in (0, 1, 2):                                       # n_call 1 falls back to one track, 3 has an odd tail
        assert {1, 3} <= {c["call"]["samples"] for c in planned if opt(c, "overlap", 0) == ov and c["call"]["kind"] == "render"}, ov
    wave_cast = [c for c in planned if opt(c, "cast_wavefront", 0) and c["plan"]["trace_form"] != "per_pixel"]
    assert any(c["lights"] == 1 for c in wave_cast)
    assert any(c["lights"] and opt(c, "slots", 1 << 29) // (c["call"]["w"] * c["call"]["h"]) < c["lights"] for c in wave_cast)
    assert {(d, s) for d in (1, 2, 3, 4, 8) for s in (False, True)} <= {(c["depth"], c["sky"]) for c in planned}
    assert any(c["call"]["kind"] == "masked" and c["call"]["mom2"] for c in planned)
    assert any(c["call"]["kind"] == "views" and c["call"]["n_views"] == 2 for c in planned)
    for kind in ("raytrace", "intersect"):
        assert {1, 2} <= {c["plan"]["variant"] for c in planned if c["call"]["kind"] == kind}, kind
    refusals = {c["refusal"].split(" needs ")[1].split(" B of ")[1].split(" per")[0] for c in GOLD["cases"] if c["refusal"] and " needs " in c["refusal"]}
    assert refusals == {"LDS", "LDS stack"}, refusals
    assert sum("exceed 2^29" in (c["refusal"] or "") for c in GOLD["cases"]) >= 1 and sum("exceed 2^31 - 1" in (c["refusal"] or "") for c in GOLD["cases"]) >= 1
    assert any("tile lanes" in (c["refusal"] or "") for c in GOLD["cases"])
    assert {c["scene"]["kind"] for c in GOLD["cases"]} == {"obj", "padded", "padded_u32", "heightfield"}


@pytest.mark.parametrize("name", list(CASES))
def test_plan_equals_the_recorded_one(sqt, name):
    """All 14 fields of sq_plan, the refusal's text and the launches the schedule implies are what the recorded commit planned."""
    case = CASES[name]
    plan, launches, refusal = run_case(sqt, case)
    assert refusal == case["refusal"]
    if case["plan"] is not None:                               # (null: refused for its size before anything was planned)
        assert plan == case["plan"]
    else:
        assert refusal and plan["launched"] == 0
    assert launches == case["trace_launches"]


def test_schedule_follows_the_slots_the_workspace_got(sqt):
    """The allocation may halve the slots: the same plan, more batches; and never fewer slots than one sample of every pixel."""
    inp, _ = case_inputs(sqt, CASES["default_8x8"])
    inp.update(k_end=8, overlap=1)
    rc, plan, full, _ = plan_call(sqt, inp)
    assert rc == 0 and (full["slots"], full["have_slots"], full["overlap"], full["n_batches"], full["batch"]) == (512, 512, 1, 2, 4)
    for have, overlap, n_batches, batch in ((256, 1, 4, 2), (128, 1, 8, 1), (64, 0, 8, 1)):
        rc, plan2, v, _ = plan_call(sqt, inp, have_slots=have)
        assert rc == 0 and plan2 == plan and (v["overlap"], v["n_batches"], v["batch"], v["n_real"]) == (overlap, n_batches, batch, n_batches), v
        check_structure(v)
        assert v["ws_total"] < full["ws_total"] and {k: v[k] for k in WS[:9]} == {k: full[k] for k in WS[:9]}     # the per-pixel arrays stay


def test_deep_block_layout(sqt):
    """oxy (8 B per slot, from depth 4 on), the trail (4 B per level and slot), tmiss behind it (under a sky): no overlap, all within
    slots x deep_slot_bytes."""
    inp, _ = case_inputs(sqt, CASES["default_8x8"])
    for depth in range(1, 9):
        for sky in (0, 1):
            rc, _, v, err = plan_call(sqt, dict(inp, depth=depth, sky=sky, deep=1))
            assert rc == 0, err
            slots = v["have_slots"]
            want = 0 if depth < 2 else (depth - 1) * 4 + (8 if depth >= 4 else 0) + (4 if sky else 0)
            assert v["deep_slot_bytes"] == want and v["need_deep"] == 1
            assert v["deep_oxy"] == 0 and v["deep_trail"] == (8 * slots if depth >= 4 else 0)
            end = v["deep_trail"] + (depth - 1) * 4 * slots
            assert v["deep_tmiss"] == (end if sky and depth >= 2 else -1)
            assert end + (4 * slots if sky and depth >= 2 else 0) == slots * want


def test_primary_grid_follows_the_tiled_enumeration(sqt):
    """The planner's copy of primary_padded (primary_padded_lanes, sq_plan.h) against the Python mirror of the kernels' own
    (tests/kernel_restatements.py): the per-lane primary pass is one thread per tile lane, the resident one strides over n_cu blocks."""
    from kernel_restatements import enumerate_pixels
    inp, _ = case_inputs(sqt, CASES["default_8x8"])
    for rows, h, tile_rows, views in ((1, 1, 8, 1), (7, 5, 1, 1), (9, 33, 1, 3), (135, 1080, 2, 1), (1080, 1920, 8, 1), (16, 31, 8, 2), (5, 640, 1, 1)):
        padded = enumerate_pixels(rows, h, tile_rows)[1]
        shape = dict(inp, local_rows=rows, h=h, tile_rows=tile_rows, tiles_x=-(-h // (64 // tile_rows)), n_views=views, source=int(views > 1))
        rc, plan, v, err = plan_call(sqt, dict(shape, primary_resident=0))
        assert rc == 0 and plan["primary_form"] == "per_lane" and v["primary_grid"] == -(-padded * views // 256) and v["primary_lds"] == v["px_lds"], (v, err)
        rc, plan, v, err = plan_call(sqt, shape)
        assert rc == 0 and plan["primary_form"] == "resident" and v["primary_grid"] == min(GOLD["n_cu"], -(-padded * views // 1024)), (v, err)


RANGES = [("variant", 0, 3, "variant must be 1 (per-pixel kernel) or 2 (wavefront)"), ("slots", 0, (1 << 29) + 1, "slots must be in 1..2^29"),
          ("straggler_lanes", -1, 64, "straggler_lanes must be in 0..63"), ("lds_node_kb", -1, 129, "lds_node_kb must be in 0..128"),
          ("trace_blocks_per_cu", -1, 9, "trace_blocks_per_cu must be in 0..8"), ("overlap", -1, 3, "overlap must be 0, 1 or 2"),
          ("rng_table_mb", -1, (1 << 20) + 1, "rng_table_mb must be in 0..2^20"), ("guided", -1, 4, "guided must be in 0..3"),
          ("aux_polite", -1, 9, "aux_polite must be in 0..8"), ("trace_prio", -1, 4, "trace_prio must be in 0..3"),
          ("descend_extra", -1, 17, "descend_extra must be in 0..16"), ("descend_lanes", 0, 65, "descend_lanes must be in 1..64"),
          ("refill_min", 0, 65, "refill_min must be in 1..64"), ("flush_min", -1, 65, "flush_min must be in 0..64"),
          ("aux_blocks_per_cu", -1, 17, "aux_blocks_per_cu must be in 0..16")]


@pytest.mark.parametrize("name,below,above,text", RANGES)
def test_option_ranges_and_their_refusals(sqt, name, below, above, text):
    """The option table: one below and one above each range is refused with the option's own text, both ends are taken."""
    inp, _ = case_inputs(sqt, CASES["default_8x8"])
    for bad in (below, above):
        rc, _, _, err = plan_call(sqt, dict(inp, **{name: bad}))
        assert rc == 2 and err == text
    for good in (below + 1, above - 1):
        assert plan_call(sqt, dict(inp, **{name: good}))[0] == 0


def test_options_without_a_range_and_unknown_names(sqt):
    inp, _ = case_inputs(sqt, CASES["default_8x8"])
    for name in ("timing", "resident", "profile", "cast_wavefront", "deep", "pool", "primary_resident", "cull", "level1_cull", "incremental",
                 "primary_tiles", "primary_pooled", "coresidency", "aux_low_priority", "pixel_major"):
        for value in (-5, 0, 1, 7):
            assert plan_call(sqt, dict(inp, **{name: value}))[0] == 0, (name, value)
    assert plan_call(sqt, dict(inp, pool=7))[1] == plan_call(sqt, dict(inp, pool=1))[1]                 # normalised to 0 / 1
    assert plan_call(sqt, dict(inp, pixel_major=-9))[2]["pixel_major"] == 0 and plan_call(sqt, dict(inp, pixel_major=5))[2]["pixel_major"] == 1
    rc, _, _, err = plan_call(sqt, dict(inp, no_such_option=1))
    assert rc == 2 and err == "unknown option 'no_such_option'"
    rc, _, _, err = plan_call(sqt, inp, outputs=["no_such_scalar"])
    assert rc == 2 and err == "no plan scalar 'no_such_scalar'"
    assert plan_call(sqt, dict(inp, n_cu=0))[0] == 2 and plan_call(sqt, dict(inp, depth=9))[0] == 2


# ---- the option tables of the GPU tests (tests/render_options.py) ----------------------------------------------------------------
# a wavefront frame, a cast frame, a ray query, a streaming form; and the last one again with 2^20 triangles, where pixel_major's
# automatic setting (-1) chooses 1.  total_rays makes chunk_rays show the option `slots` itself, not the slots a small frame wants.
TABLE_CASES = (("default_8x8", {}), ("cast", {}), ("intersect", {}), ("u16_height46_8x8", {}), ("u16_height46_8x8", {"n_tris": 1 << 20}))
EVERY_SCALAR = OUT + WS + ["nonneg_materials", "n_emitters", "cull_off"]
OTHER_VALUES = {"variant": (1,), "resident": (0,), "profile": (1,), "overlap": (1, 2), "primary_pooled": (1,), "pool": (0,), "slots": (64, 100),
                "cull": (0,), "trace_blocks_per_cu": (1, 2, 3), "primary_resident": (0,), "pixel_major": (0, 1), "cast_wavefront": (1,)}


def test_every_option_table_of_the_gpu_tests_states_the_librarys_defaults(sqt):
    """An option that is not given takes its default (Options, csrc/sq_plan.h).  So a table states the defaults exactly when planning
    with its keys given equals planning with none, on the plan and every scalar the window shows; and a key counts only if the
    plan shows it: some other value of it changes some output of some case."""
    import render_options as RO
    keys = set().union(*RO.TABLES.values())
    assert keys == set(OTHER_VALUES) and not keys & {"timing", "rng_table_mb", "aux_low_priority"}
    base = []
    for name, changed in TABLE_CASES:
        inp, rays = case_inputs(sqt, CASES[name])
        assert rays is None and not CASES[name]["options"]
        inp = dict(inp, total_rays=1 << 30, **changed)
        want = plan_call(sqt, inp, outputs=EVERY_SCALAR)[:3]
        assert want[0] == 0
        for tname, table in RO.TABLES.items():
            assert plan_call(sqt, {**inp, **table}, outputs=EVERY_SCALAR)[:3] == want, (tname, name)
        base.append((inp, want))
    for key, values in OTHER_VALUES.items():
        assert any(plan_call(sqt, {**inp, key: v}, outputs=EVERY_SCALAR)[:3] != want for inp, want in base for v in values), key
