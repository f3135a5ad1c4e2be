"""The automatic schedule of the call planner (csrc/sq_plan_call.h: plan_schedule) through sq_plan_call, on the CPU.

With option "overlap" 0 and "auto_overlap" 1 a call of the three-level pipeline is planned as two pipelines once it has two samples, its
workspace holds two samples of every pixel and pixels x samples reaches "auto_overlap_slots"; under option "mirror_ride" the mirror rays
then ride at the head of batch 0's first trace launch.  Held here: the rule at each of its edges, the batch arithmetic (multiples of four samples from eight
samples on, "batches_per_track"), that "overlap" 1 and 2 plan what they always planned -- against a restatement of the planner's
arithmetic before the automatic schedule existed -- and that no recorded default-option case overlaps.
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
OUT = ["path", "pixels", "n_call", "slots", "have_slots", "schedule", "mirror_rides", "overlap", "tracks", "track_slots", "batch", "n_batches",
       "n_real", "tail_kc"]
PIPELINE = 5
SERIAL, AUX, PIPELINES = 0, 1, 2
DEFAULT_THRESHOLD = 1 << 26


def plan(sqt, inputs, have_slots=0):
    """sq_plan_call: the OUT scalars of a call that must plan."""
    L = sqt.lib()
    names = (C.c_char_p * len(inputs))(*[k.encode() for k in inputs])
    values = (C.c_int64 * len(inputs))(*[int(v) for v in inputs.values()])
    onames = (C.c_char_p * len(OUT))(*[k.encode() for k in OUT])
    ovalues = (C.c_int64 * len(OUT))()
    p = sqt._native.Plan()
    rc = L.sq_plan_call(names, values, len(inputs), have_slots, C.byref(p), onames, ovalues, len(OUT))
    assert rc == 0, L.sq_last_error().decode()
    return dict(zip(OUT, [int(v) for v in ovalues]))


@pytest.fixture(scope="module")
def scene(sqt):
    """The planner's scene inputs of data/scene.obj, from the packer on the CPU."""
    holder, L, h = R.scene_of(sqt, CASES["default_8x8"]["scene"]), sqt.lib(), C.c_void_p()
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
    return dict(out, n_cu=GOLD["n_cu"])


def frame(scene, w, h, n, k_begin=0, **opts):
    return dict(scene, source=0, local_rows=w, h=h, tile_rows=8, tiles_x=-(-h // 8), k_begin=k_begin, k_end=k_begin + n, **opts)


def check_structure(v):
    """test_plan.check_structure's invariants on the schedule scalars, and what the two new ones add."""
    assert 1 <= v["n_real"] <= v["n_batches"] and v["batch"] * v["n_batches"] >= v["n_call"] >= 1, v
    assert v["batch"] * v["pixels"] <= v["track_slots"] and v["tracks"] * v["track_slots"] <= v["have_slots"], v
    assert v["tracks"] == 1 + v["overlap"] and (v["n_real"] - 1) * v["batch"] + v["tail_kc"] == v["n_call"], v
    assert 1 <= v["tail_kc"] <= v["batch"], v
    assert v["overlap"] == int(v["schedule"] != SERIAL) and v["schedule"] in (SERIAL, AUX, PIPELINES), v
    if v["schedule"] == SERIAL:
        assert v["mirror_rides"] == 1, v
    else:
        assert v["n_real"] >= 2, v


def old_schedule(overlap, path, pixels, n_call, have):
    """plan_schedule before the automatic schedule, restated: (overlap, tracks, track_slots, batch, n_batches, n_real)."""
    ov = int(bool(overlap) and path == PIPELINE and n_call >= 2 and have >= 2 * pixels)
    tracks = 1 + ov
    track_slots = have // tracks
    max_batch = max(1, min(n_call, track_slots // pixels))
    n_batches = max(tracks, -(-n_call // max_batch))
    batch = -(-n_call // n_batches)
    n_real = sum(1 for i in range(n_batches) if min(batch, n_call - i * batch) > 0)
    return ov, tracks, track_slots, batch, n_batches, n_real


def is_old(v, overlap):
    return (v["overlap"], v["tracks"], v["track_slots"], v["batch"], v["n_batches"], v["n_real"]) == \
        old_schedule(overlap, v["path"], v["pixels"], v["n_call"], v["have_slots"])


def test_the_default_threshold_and_the_rule_at_its_edges(scene, sqt):
    # the library's default: one slot below it and at it (2^13 x 2^13 pixels at one sample below would need n_call 1: use 2^25 pixels x 2)
    w, h = 1 << 12, 1 << 13
    at = plan(sqt, frame(scene, w, h, 2))
    assert at["pixels"] * at["n_call"] == DEFAULT_THRESHOLD and (at["schedule"], at["mirror_rides"], at["tracks"]) == (PIPELINES, 0, 2), at
    check_structure(at)
    below = plan(sqt, frame(scene, w, h - 1, 2))
    assert below["pixels"] * below["n_call"] < DEFAULT_THRESHOLD and below["schedule"] == SERIAL and is_old(below, 0), below
    # a threshold of its own: 8 x 8 @ 4 has 256 slots
    for thr, want in ((257, SERIAL), (256, PIPELINES), (1, PIPELINES)):
        v = plan(sqt, frame(scene, 8, 8, 4, auto_overlap_slots=thr))
        assert v["schedule"] == want and v["mirror_rides"] == int(want == SERIAL), (thr, v)
        check_structure(v)
    # one sample; a workspace one slot short of two samples of every pixel
    v = plan(sqt, frame(scene, 8, 8, 1, auto_overlap_slots=1))
    assert v["schedule"] == SERIAL and is_old(v, 0), v
    v = plan(sqt, frame(scene, 8, 8, 4, auto_overlap_slots=1), have_slots=127)
    assert v["schedule"] == SERIAL and is_old(v, 0) and v["batch"] == 1, v
    v = plan(sqt, frame(scene, 8, 8, 4, auto_overlap_slots=1), have_slots=128)
    assert (v["schedule"], v["batch"], v["n_real"], v["track_slots"]) == (PIPELINES, 1, 4, 64), v
    check_structure(v)
    # the option off: the serial schedule, whatever the threshold
    v = plan(sqt, frame(scene, 8, 8, 4, auto_overlap_slots=1, auto_overlap=0))
    assert v["schedule"] == SERIAL and is_old(v, 0), v


def test_cast_and_deep_paths_stay_serial(scene, sqt):
    for extra in (dict(depth=4), dict(depth=2), dict(deep=1), dict(sky=1), dict(cast=1, cast_wavefront=1, n_lights=4, lights_set=1)):
        v = plan(sqt, frame(scene, 8, 8, 4, auto_overlap_slots=1, **extra))
        assert v["path"] != PIPELINE and v["schedule"] == SERIAL and v["mirror_rides"] == 1 and v["tracks"] == 1, (extra, v)
        assert is_old(v, 0), (extra, v)


@pytest.mark.parametrize("overlap", [1, 2])
def test_explicit_overlap_plans_what_it_planned(scene, sqt, overlap):
    """Whatever the automatic options say: the old arithmetic, no alignment, the mirror rays in a launch of their own."""
    for n in (1, 2, 3, 7, 8, 9, 250, 256):
        for have in (0, 64, 127, 128, 200, 64 * 9):
            for auto in (dict(), dict(auto_overlap_slots=1, batches_per_track=4), dict(auto_overlap=0)):
                v = plan(sqt, frame(scene, 8, 8, n, overlap=overlap, **auto), have_slots=have)
                assert is_old(v, overlap), (n, have, auto, v)
                assert v["schedule"] == (overlap if v["overlap"] else SERIAL) and v["mirror_rides"] == 1 - v["overlap"], v
                check_structure(v)


@pytest.mark.parametrize("n_call,batches", [(2, [1, 1]), (3, [1, 1, 1]), (5, [2, 2, 1]), (7, [3, 3, 1]), (8, [4, 4]), (9, [4, 4, 1]), (12, [4, 4, 4]),
                                            (250, [124, 124, 2]), (256, [128, 128])])
def test_batches_of_the_automatic_schedule(scene, sqt, n_call, batches):
    """A call wants one slot per sample, so a track holds half its samples, rounded down.  From eight samples on a batch is a multiple of
    four and only the last one is ragged; below, the even split of what a track holds."""
    v = plan(sqt, frame(scene, 8, 8, n_call, auto_overlap_slots=1))
    check_structure(v)
    got = [min(v["batch"], n_call - i * v["batch"]) for i in range(v["n_real"])]
    assert v["schedule"] == PIPELINES and got == batches, (v, got)
    # a sample range that starts at 3 is the same schedule
    v3 = plan(sqt, frame(scene, 8, 8, n_call, k_begin=3, auto_overlap_slots=1))
    assert {k: v3[k] for k in OUT} == {k: v[k] for k in OUT}


def test_slots_that_force_several_batches_per_track(scene, sqt):
    """The workspace bounds a batch: a track of four samples gives batches of four, a smaller track cannot align."""
    for n_call, slots, batch, n_real in ((256, 64 * 8, 4, 64), (250, 64 * 8, 4, 63), (250, 64 * 40, 20, 13), (9, 64 * 8, 4, 3),
                                         (9, 64 * 6, 3, 3), (5, 128, 1, 5), (256, 64 * 20, 8, 32), (23, 64 * 18, 8, 3)):
        v = plan(sqt, frame(scene, 8, 8, n_call, auto_overlap_slots=1, slots=slots))
        check_structure(v)
        assert (v["schedule"], v["batch"], v["n_real"]) == (PIPELINES, batch, n_real), (n_call, slots, v)
        if n_call >= 8 and slots >= 64 * 8:
            assert v["batch"] % 4 == 0, v


def test_batches_per_track(scene, sqt):
    for n_call, per, batch, n_real in ((256, 1, 128, 2), (256, 2, 64, 4), (256, 4, 32, 8), (250, 4, 32, 8), (6, 2, 2, 3), (6, 4, 1, 6),
                                       (2, 4, 1, 2), (8, 4, 4, 2)):
        v = plan(sqt, frame(scene, 8, 8, n_call, auto_overlap_slots=1, batches_per_track=per))
        check_structure(v)
        assert (v["schedule"], v["batch"], v["n_real"]) == (PIPELINES, batch, n_real), (n_call, per, v)
    L = sqt.lib()
    for bad in (0, 65):
        inputs = frame(scene, 8, 8, 4, batches_per_track=bad)
        names = (C.c_char_p * len(inputs))(*[k.encode() for k in inputs])
        values = (C.c_int64 * len(inputs))(*[int(x) for x in inputs.values()])
        assert L.sq_plan_call(names, values, len(inputs), 0, C.byref(sqt._native.Plan()), None, None, 0) == 2
        assert L.sq_last_error().decode() == "batches_per_track must be in 1..64"


def test_mirror_ride_is_an_option_of_the_automatic_schedule(scene, sqt):
    """The automatic schedule with the mirror rays at the head of batch 0's first launch: the same batches, mirror_rides 1."""
    a, b = (plan(sqt, frame(scene, 8, 8, 9, auto_overlap_slots=1, mirror_ride=m)) for m in (1, 0))
    assert (a["mirror_rides"], b["mirror_rides"]) == (1, 0) and {k: a[k] for k in OUT if k != "mirror_rides"} == {k: b[k] for k in OUT if k != "mirror_rides"}
    assert plan(sqt, frame(scene, 8, 8, 9, auto_overlap_slots=1))["mirror_rides"] == 0                # the default: a launch of their own
    assert plan(sqt, frame(scene, 8, 8, 9, auto_overlap=0, mirror_ride=0))["mirror_rides"] == 1     # the serial schedule has no other place for them
    for overlap in (1, 2):                                                                         # nor do the schedules a caller asks for read it
        assert plan(sqt, frame(scene, 8, 8, 9, overlap=overlap, mirror_ride=1))["mirror_rides"] == 0


def test_no_recorded_case_changes_its_schedule(scene, sqt):
    """Every recorded frame of data/scene.obj, under the library's default threshold: a default-option case stays serial, an explicit
    overlap plans the old arithmetic (tests/test_plan.py holds the plans themselves to the recording)."""
    seen = set()
    for case in GOLD["cases"]:
        c, opts = case["call"], case["options"]
        if case["scene"] != CASES["default_8x8"]["scene"] or c["kind"] != "render" or case["plan"] is None or case["refusal"]:
            continue
        inp = frame(scene, c["w"], c["h"], c["samples"], **opts)
        inp.update(cast=int(c["cast"]), depth=case["depth"] or 3, sky=int(case["sky"]), lights_set=int(case["lights"] is not None),
                   n_lights=case["lights"] or 1)
        if not opts.get("primary_tiles", 1):
            inp.update(tile_rows=1, tiles_x=-(-c["h"] // 64))
        v = plan(sqt, inp)
        if v["slots"] == 0:
            continue
        overlap = opts.get("overlap", 0)
        assert is_old(v, overlap), (case["name"], v)
        assert v["schedule"] == (overlap if v["overlap"] else SERIAL) and v["mirror_rides"] == 1 - v["overlap"], (case["name"], v)
        seen.add(v["schedule"])
    assert seen == {SERIAL, AUX, PIPELINES}
