"""The link between the library's kernels and the kernel walk (tests/kernel_walk.py), on the CPU.

tests/golden/kernel_walk.json records, from a kernel trace of the walk on an MI355X (tools/kernel_walk_trace.py), which case dispatched
which kernel.  Here: (a) the kernels of the built library's gfx950 code objects -- their names from the ELF symbol tables, nothing
else of them is read -- are exactly the file's kernels plus kernel_walk.UNREACHABLE, so a new or renamed instantiation fails until a
case launches it and the file is recorded again; (b) the file and CASES agree, and every case was seen dispatching all it claims;
(c) UNREACHABLE is what the planner cannot choose, shown through sq_plan_call; (d) CASES is deterministic and claims only what exists."""
import ctypes as C
import json
import os
import sys

import pytest

import kernel_walk as KW
import scenes as SC
import tree_padding as TP
from conftest import DATA, GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_walk_trace as KT  # noqa: E402

GOLD = json.load(open(os.path.join(GOLDEN, "kernel_walk.json")))
LDS = 160 * 1024


# ---- (a) ---------------------------------------------------------------------------------------------------------------------
def test_the_librarys_kernels_are_the_recorded_ones_plus_the_unreachable_ones(sqt):
    lib = KT.kernel_symbols(sqt.LIB_PATH)
    launched = [k["mangled"] for k in GOLD["kernels"]]
    unreachable = [k["mangled"] for k in GOLD["unreachable"]]
    assert len(set(launched)) == len(launched) and len(set(unreachable)) == len(unreachable) and not set(launched) & set(unreachable)
    assert sorted(k["name"] for k in GOLD["unreachable"]) == sorted(KW.UNREACHABLE)
    new = sorted(set(lib) - set(launched) - set(unreachable))
    gone = sorted((set(launched) | set(unreachable)) - set(lib))
    assert not new, f"kernels no case of tests/kernel_walk.py is recorded launching (add a case, record tests/golden/kernel_walk.json again): {new}"
    assert not gone, f"recorded kernels the library no longer has (record tests/golden/kernel_walk.json again): {gone}"
    assert len(lib) == len(launched) + len(unreachable)
    print(f"[kernel walk] {len(lib)} kernels: {len(launched)} launched, {len(unreachable)} unreachable")


# ---- (b) ---------------------------------------------------------------------------------------------------------------------
def test_every_recorded_kernel_has_a_case_and_every_case_was_seen_dispatching_what_it_claims():
    by_name = {k["name"]: k for k in GOLD["kernels"]}
    assert len(by_name) == len(GOLD["kernels"])
    names = set(KW.NAMES)
    for k in GOLD["kernels"]:
        assert k["cases"], k["name"]
        assert set(k["cases"]) <= names, (k["name"], sorted(set(k["cases"]) - names))
    assert GOLD["n_cases"] == len(KW.CASES)
    for c in KW.CASES:
        for claim in c.claims:
            assert claim in by_name and c.name in by_name[claim]["cases"], (c.name, claim)
    assert {n for k in GOLD["kernels"] for n in k["cases"]} == names       # no case without a kernel of the library


# ---- (c) ---------------------------------------------------------------------------------------------------------------------
def plan(sqt, **inputs):
    """sq_plan_call of a camera frame (or what `inputs` says) on a scene given by its scalars: (return code, trace form, primary form, resident)."""
    base = dict(n_verts=0, height=0, trix=1, packed_leaves=1, n_emitters=0, nonneg_materials=1, finite_geometry=1, shortcut_depth=8, level1_on=0,
                n_cu=256, depth=3, source=0, local_rows=8, h=8, tile_rows=8, tiles_x=1, k_begin=0, k_end=2, resident=1)
    base.update(inputs)
    N, L = sqt._native, sqt.lib()
    names = (C.c_char_p * len(base))(*[k.encode() for k in base])
    values = (C.c_int64 * len(base))(*[int(v) for v in base.values()])
    onames = (C.c_char_p * 1)(b"resident")
    ovalues = (C.c_int64 * 1)()
    p = N.Plan()
    rc = L.sq_plan_call(names, values, len(base), 0, C.byref(p), onames, ovalues, 1)
    return rc, N.TRACE_FORMS[p.trace_form], N.PRIMARY_FORMS[p.primary_form], int(ovalues[0])


CALLS = ({}, {"pool": 0}, {"profile": 1}, {"source": 1, "n_views": 2}, {"source": 2, "local_rows": 1, "tile_rows": 1}, {"masked": 1, "mom2": 1},
         {"sky": 1, "depth": 4}, {"cast": 1, "cast_wavefront": 1}, {"query": 1, "n_rays": 64}, {"primary_pooled": 1}, {"lds_node_kb": 128})


@pytest.mark.parametrize("call", CALLS, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()) or "frame")
def test_no_call_plans_the_resident_form_for_a_scene_with_4_byte_stack_words(sqt, call):
    """4-byte words mean n_branches >= 0x8000 or n_tris >= 0x8000 (the packer; below).  At either boundary, the other count at 1 and
    the fewest vertices and the lowest tree a scene can have, no call plans the resident form, and the layout only grows with the counts.
    With 2-byte words the same calls do plan it, up to counts well below the boundary: the difference is the scene, not the call."""
    for nb, nt in ((0x8000, 1), (1, 0x8000), (0x8000, 0x8000), (0x9000, 6238), (1 << 20, 1 << 20)):
        rc, form, primary, resident = plan(sqt, small_index=0, n_branches=nb, n_tris=nt, **call)
        assert rc == 0 and form != "resident" and primary != "resident" and resident == 0, (nb, nt, form, primary)
    rc, form, primary, resident = plan(sqt, small_index=1, n_branches=1, n_tris=1, **call)
    assert rc == 0 and form == "resident" and resident == 1, (form, primary)
    if not call.get("query") and not call.get("primary_pooled"):
        assert primary == "resident"
    for key in ("n_branches", "n_tris"):                               # the largest count that still plans resident is far below 0x8000
        lo, hi = 1, 0x8000
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if plan(sqt, small_index=1, **{"n_branches": 1, "n_tris": 1, key: mid}, **call)[1] == "resident":
                lo = mid
            else:
                hi = mid
        assert plan(sqt, small_index=1, **{"n_branches": 1, "n_tris": 1, key: 0x7FFF}, **call)[1] != "resident"
        assert lo < LDS // (32 if key == "n_branches" else 8) < 0x8000, (key, lo)


def test_the_packer_gives_4_byte_words_exactly_from_0x8000_branches_on(sqt):
    bih = sqt.BIH(sqt.Mesh.from_obj(os.path.join(DATA, "scene.obj"), DATA))
    nb0 = int(((bih.nodes["kind"] & 3) != 3).sum())
    for target, small in ((0x7FFF, 1), (0x8000, 0)):
        ps = TP.PaddedScene(bih, {0: [(0, TP.LEFT, ("balanced", target - nb0 - 1))]})
        assert ps.n_branches == target
        assert SC.pack(sqt, ps)[1]["small_index"] == small


def test_unreachable_is_every_resident_scene_kernel_with_4_byte_words_and_nothing_else():
    names = [k["name"] for k in GOLD["kernels"]] + [k["name"] for k in GOLD["unreachable"]]
    resident_u32 = sorted(n for n in names if n.startswith("sq_primary_resident<unsigned int,") or n.startswith("sq_trace_rays<unsigned int, true,"))
    assert resident_u32 == sorted(KW.UNREACHABLE) and len(KW.UNREACHABLE) == 12
    assert sorted(k["name"] for k in GOLD["unreachable"]) == sorted(KW.UNREACHABLE)


# ---- what the cases' inputs show ---------------------------------------------------------------------------------------------
def test_the_frames_lights_and_rays_of_the_walk_can_tell_a_wrong_kernel(sqt, O):
    """Equal outputs mean little where everything is black: the two square-ish frames hit and miss the scene under both cameras, every
    light lights and shadows hit pixels, most hit pixels and rays carry radiance, a sky changes every missing pixel, depth 8 is not
    depth 3; the narrow frame is the all-miss frame it is documented as."""
    import numpy as np
    w = KW.Walk()
    for cam in ("camera", "rotated"):
        for frame in (KW.F8, KW.FE):
            rows, cols, _ = frame
            rays = [O.make_ray(rows, cols, y, x, w.ocam[cam]) for y in range(rows) for x in range(cols)]
            for n in (3, 5):
                _, lit = w.restatement.radiance((cam, rows, cols), rays, KW.lights_of(n))
                hit = int((lit[:, 0] >= 0).sum())
                assert rows * cols // 4 <= hit <= rows * cols * 3 // 4, (cam, frame, hit)
                assert ((lit == 1).sum(0) >= 10).all() and ((lit == 0).sum(0) >= 2).all(), (cam, frame, n)
            avg3 = w.want_path_frame(cam, frame, 3, None)[2]
            avg8 = w.want_path_frame(cam, frame, 8, None)[2]
            sky = w.want_path_frame(cam, frame, 4, KW.SKY)[2]
            assert (avg3 != 0).any(-1).sum() >= hit * 0.9 and (avg8 != avg3).any(-1).sum() >= hit // 4, (cam, frame)
            assert (sky != 0).all() and len(np.unique(w.want_path_frame(cam, frame, 3, None)[3].reshape(-1, 3), axis=0)) >= 20, (cam, frame)
        assert not w.want_path_frame(cam, KW.F370, 3, None)[2].any() and (w.want_path_frame(cam, KW.F370, 4, KW.SKY)[2] != 0).all()
    for frame in (KW.F8, KW.FE):
        total = w.want_raytrace(frame, 3, None)[0]
        tri = w.want_hits(frame)[0]
        assert len(total) // 3 <= (tri >= 0).sum() <= len(total) * 3 // 4 and (total != 0).any(-1).sum() >= (tri >= 0).sum() * 0.9, frame
        assert (w.want_raycast(frame, 5) != 0).any(-1).sum() >= (tri >= 0).sum() // 2, frame
        _, _, s = w.rays(frame)
        assert (s < 0).sum() >= 20 and (s > 1 << 40).sum() >= 20 and ((s >= 0) & (s < 1 << 20)).sum() >= 20


# ---- (d) ---------------------------------------------------------------------------------------------------------------------
def test_the_cases_are_deterministic_and_claim_only_kernels_of_the_library():
    assert len(set(KW.NAMES)) == len(KW.NAMES)
    again = KW._cases()
    assert [c.name for c in again] == KW.NAMES and [c.claims for c in again] == [c.claims for c in KW.CASES]
    names = {k["name"] for k in GOLD["kernels"]}
    for c in KW.CASES:
        assert c.claims and set(c.claims) <= names, (c.name, sorted(set(c.claims) - names))
        assert not set(c.claims) & set(KW.UNREACHABLE), c.name
    assert {k for c in KW.CASES for k in c.claims} == names            # every launched kernel is claimed by a case written for it
