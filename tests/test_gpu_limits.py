"""The trace kernels at the limits where their layout changes: stack depth (per form and word width), the 16-bit stack
word, the resident form's LDS budget and vertex limit, packed leaves, the emitter list, and the streaming tunables.

The oracle builds its own tree, so tall trees and exact node counts come from transparent padding (tests/tree_padding.py):
the oracle's image of the unpadded scene is the exact expected image of the padded one (tests/test_tree_padding.py checks
that premise on the CPU).  Every render is compared bit for bit (avg bits and RGB8).  DeviceScene.last_plan() shows which
side of each limit a render is on; pytest -s prints one line per boundary.
"""
import os

import numpy as np
import pytest

import tree_padding as TP
from bitcmp import bits
from conftest import DATA, GOLDEN
from render_options import THREADS
from scenes import LIMITS_H as H, LIMITS_W as W, big_leaf as _big_leaf, near_of, oracle_tris as _oracle_tris, tall_u32 as _tall_u32

pytestmark = pytest.mark.gpu
SPP = 2
LDS = 160 * 1024


@pytest.fixture(scope="module")
def base(sqt, O):
    bih = sqt.BIH(sqt.Mesh.from_obj(os.path.join(DATA, "scene.obj"), DATA))
    ob = O.BIH(O.tris_from_obj(os.path.join(DATA, "scene.obj"), DATA))
    cam_p, cam_o = sqt.load_camera(os.path.join(DATA, "camera")), O.load_camera(os.path.join(DATA, "camera"))
    exp = {cast: ob.render(cam_o, 1 if cast else SPP, W, H, cast=cast, threads=THREADS)[:2] for cast in (False, True)}
    return bih, cam_p, exp, near_of(O, cam_o)


def render(ds, cam, spp, w, h, cast=False):
    import torch
    a, r = ds.render_rows(cam, spp, w, h, cast=cast)
    torch.cuda.synchronize()
    return a.cpu().numpy(), r.cpu().numpy()


def probe(sqt, scene, cam, opts):
    """(plan, None) of a 1 x 1 frame at 1 spp under opts, or (plan so far, error message) when the frame is refused."""
    ds = sqt.DeviceScene(scene, 0)
    try:
        for k, v in opts.items():
            ds.set_option(k, v)
        try:
            render(ds, cam, 1, 1, 1)
            return ds.last_plan(), None
        except sqt.SquiglyError as e:
            plan = ds.last_plan()
            assert plan["launched"] == 0
            return plan, str(e)
    finally:
        ds.close()


def check_frame(sqt, scene, cam, exp, opts, casts=(False, True), culls=(0, 1)):
    """Render under opts (both cull settings, a path-traced and a cast frame) and compare with the expected images; returns the plan."""
    ds = sqt.DeviceScene(scene, 0)
    plan = None
    try:
        for k, v in opts.items():
            ds.set_option(k, v)
        for cull in culls:
            ds.set_option("cull", cull)
            for cast in casts:
                a, r = render(ds, cam, 1 if cast else SPP, W, H, cast=cast)
                ea, er = exp[cast]
                assert np.array_equal(bits(a), bits(ea)), (opts, cull, cast, int((bits(a) != bits(ea)).any(-1).sum()))
                assert np.array_equal(r, er), (opts, cull, cast)
                if not cast:
                    plan = ds.last_plan()
    finally:
        ds.close()
    return plan


def key_of(plan, err):
    return "refused" if err else plan["trace_form"]


FORMS = ["resident", "streaming_six_wave", "streaming_plain", "per_pixel", "refused"]


# Measured on the MI355X: the largest height of each form, per stack word and launch options, before the next form (or the
# refusal).  The forms change where include/squigly_hip.h (sq_scene.height) says they do.
EXPECT = {
    2: {"variant1": [("per_pixel", 320)],
        "default": [("resident", 13), ("streaming_six_wave", 46), ("streaming_plain", 158)],
        "plain": [("resident", 13), ("streaming_plain", 158)],
        "stream_only": [("streaming_six_wave", 46), ("streaming_plain", 158)],
        "pool0": [("resident", 14), ("streaming_plain", 159)]},
    4: {"variant1": [("per_pixel", 160)],
        "default": [("streaming_six_wave", 23), ("streaming_plain", 79)],
        "plain": [("streaming_plain", 79)],
        "stream_only": [("streaming_six_wave", 23), ("streaming_plain", 79)],
        "pool0": [("streaming_plain", 79)]},
}
CONFIGS = {"variant1": {"variant": 1}, "default": {}, "plain": {"trace_blocks_per_cu": 2}, "stream_only": {"resident": 0},
           "pool0": {"pool": 0}}


@pytest.mark.parametrize("word", [2, 4])
def test_height_limits_per_form(sqt, O, base, word):
    """Step the root chain to each form's largest accepted height, the first height where the form changes and the first
    height refused; render bit-equal on both sides of every change (both primary-ray forms too).  uint32_t frames: scene.obj
    under an empty subtree that takes the branch count to 0x9000, so that the scene's own deepest branches have indices
    above 0x8000 and are pushed as frames."""
    bih0, cam, exp, (axis, side) = base
    cache = {}

    def ps_of(h):
        if h not in cache:
            cache[h] = TP.full_stack(bih0, h, axis, side) if word == 2 else _tall_u32(bih0, h, axis, side)
        return cache[h]
    h0 = bih0.height if word == 2 else bih0.height + 9
    if word == 4:
        ps = ps_of(h0)
        assert ps.n_branches == 0x9000 and ps.height == h0
        num, _ = TP.bfs_branch_numbers(ps.nodes)
        n = len(bih0.nodes)
        start = [i for i in range(len(ps.nodes) - n + 1)
                 if np.array_equal(ps.nodes["kind"][i:i + n], bih0.nodes["kind"]) and np.array_equal(ps.nodes["lmax"][i:i + n], bih0.nodes["lmax"])]
        assert len(start) == 1
        assert (num[start[0]:start[0] + n] > 0x8000).sum() > 100    # the scene's own deep branches
        plan = check_frame(sqt, ps, cam, exp, {"variant": 1}, casts=(False,))   # frames of branches >= 0x8000: images first
        assert plan["stack_word_bytes"] == 4
    measured = {}
    for name, opts in CONFIGS.items():
        plan0, err0 = probe(sqt, ps_of(h0), cam, opts)
        assert err0 is None and plan0["stack_word_bytes"] == word, (name, err0, plan0)
        h, key = h0, key_of(plan0, err0)
        measured[name] = []
        while key != "refused":
            lo, hi = h, h + 1                            # bracket the next form change, then bisect it
            while key_of(*probe(sqt, ps_of(hi), cam, opts)) == key:
                assert hi < 400, (name, key)
                lo, hi = hi, min(hi * 2, 400)
            while hi - lo > 1:
                mid = (lo + hi) // 2
                if key_of(*probe(sqt, ps_of(mid), cam, opts)) == key:
                    lo = mid
                else:
                    hi = mid
            plan_hi, err_hi = probe(sqt, ps_of(hi), cam, opts)
            nkey = key_of(plan_hi, err_hi)
            assert FORMS.index(nkey) > FORMS.index(key), (name, key, nkey)
            # primary rays: as the form chooses, one ray per lane, and through the pooled trace kernel (where each applies)
            pooled = opts.get("pool", 1) != 0
            variants = [(dict(opts), None)]
            if key == "resident":
                variants.append((dict(opts, primary_resident=0), "per_lane"))
            if key != "per_pixel" and pooled:
                variants.append((dict(opts, primary_pooled=1), "pooled"))
            for i, (v, prim) in enumerate(variants):     # both sides, bit-equal: the last height of the form, the first of the next
                plan_lo = check_frame(sqt, ps_of(lo), cam, exp, v, casts=(False, True) if i == 0 else (False,))
                assert plan_lo["trace_form"] == key and plan_lo["stack_cap"] == lo and plan_lo["stack_word_bytes"] == word, plan_lo
                want = prim or {"per_pixel": "none", "resident": "resident"}.get(key, "per_lane")
                assert plan_lo["primary_form"] == want, (v, plan_lo)
                if i == 0:
                    first = plan_lo
                if err_hi is None:
                    plan_hi = check_frame(sqt, ps_of(hi), cam, exp, v, casts=(False,))
                    assert plan_hi["trace_form"] == nkey and plan_hi["primary_form"] == (prim or ("resident" if nkey == "resident" else "per_lane")), (v, plan_hi)
            if err_hi is not None:                        # refused on the host, before any launch
                assert f"BIH height {hi} needs" in err_hi, err_hi
            print(f"[limits] u{8 * word} {name}: {key} up to height {lo} ({first['trace_lds_bytes']} B trace LDS, "
                  f"{first['pixel_lds_bytes']} B per-pixel LDS, {first['blocks_per_cu']} workgroups per CU), then {nkey} at {hi}"
                  + (f": {err_hi}" if err_hi else ""))
            measured[name].append((key, lo))
            if key == "per_pixel":
                assert first["pixel_lds_bytes"] == 256 * lo * word and first["pixel_lds_bytes"] > 64 * 1024
            h, key = hi, nkey
    assert measured == EXPECT[word]
    # the device is still sound: a fresh scene gives the golden frame
    ds = sqt.DeviceScene(bih0, 0)
    try:
        a, r = render(ds, cam, 4, 64, 64)
    finally:
        ds.close()
    assert np.array_equal(bits(a), bits(np.load(os.path.join(GOLDEN, "scene_64x64_4spp_avg.npy"))))
    assert np.array_equal(r, np.load(os.path.join(GOLDEN, "scene_64x64_4spp_rgb8.npy")))


def test_branch_count_word_boundary(sqt, base):
    """Exactly 0x7FFF and 0x8000 branches, reached with a balanced empty subtree beside the scene (same height and same
    trace form on both sides): uint16_t frames, then uint32_t."""
    bih0, cam, exp, (axis, side) = base
    nb0 = int(((bih0.nodes["kind"] & 3) != 3).sum())
    forms = set()
    for target, word in ((0x7FFF, 2), (0x8000, 4)):
        ps = TP.PaddedScene(bih0, {0: [(axis, side, ("balanced", target - nb0 - 1))]})
        assert ps.n_branches == target
        plan = check_frame(sqt, ps, cam, exp, {}, casts=(False, True))
        assert plan["stack_word_bytes"] == word
        forms.add((ps.height, plan["trace_form"]))
        check_frame(sqt, ps, cam, exp, {"variant": 1}, casts=(False,), culls=(0,))
        print(f"[limits] {target:#x} branches (height {ps.height}): {word} B stack words, {plan['trace_form']}")
    assert len(forms) == 1, forms


def test_triangle_count_word_boundary(sqt, O):
    """Exactly 0x7FFF and 0x8000 triangles (a random soup): uint16_t frames, then uint32_t; triangles with flattened
    index >= 0x7F00 are hit by primary rays."""
    cam_txt = b"-6 0.1 0.2\n0 0 0\n"
    cam_p, cam_o = sqt.camera_from_text(cam_txt), O.camera_from_text(cam_txt)
    mats = np.zeros(3, sqt._native.MAT_DTYPE)
    mats["reflective"] = [0.0, 0.5, 0.0]
    mats["surf"] = [[0.7, 0.6, 0.5], [0.4, 0.8, 0.6], [0, 0, 0]]
    mats["emissive"] = [0, 0, 30]
    mats["emit"] = [[0, 0, 0], [0, 0, 0], [1.0, 0.9, 0.7]]
    for n, word in ((0x7FFF, 2), (0x8000, 4)):
        rng = np.random.default_rng(n)
        c = rng.uniform(-1.5, 1.5, (n, 1, 3))
        c[..., 0] *= 0.1                                  # a thick wall facing the camera: every part of the tree is in view
        v = (c + rng.normal(0, 0.08, (n, 3, 3))).astype(np.float32)
        tris = np.zeros(n, sqt._native.TRI_DTYPE)
        tris["v0"], tris["v1"], tris["v2"] = v[:, 0], v[:, 1], v[:, 2]
        tris["mat"] = rng.choice(3, n, p=[0.8, 0.15, 0.05])
        bih = sqt.BIH(sqt.Mesh.from_arrays(tris, mats))
        ob = O.BIH(_oracle_tris(O, tris, mats))
        assert bih.scene.n_tris == n
        hits = {ob.intersect(*O.make_ray(64, 64, y, x, cam_o)).tri for y in range(64) for x in range(64)}
        assert max(hits) >= 0x7F00, max(hits)
        exp = {cast: ob.render(cam_o, 1 if cast else SPP, W, H, cast=cast, threads=THREADS)[:2] for cast in (False, True)}
        plan = check_frame(sqt, bih, cam_p, exp, {}, culls=(0, 1))
        assert plan["stack_word_bytes"] == word
        check_frame(sqt, bih, cam_p, exp, {"variant": 1}, casts=(False,), culls=(0,))
        print(f"[limits] {n:#x} triangles: {word} B stack words, {plan['trace_form']}, "
              f"{sum(t >= 0x7F00 for t in hits)} primary-hit triangles at index >= 0x7f00")


def test_resident_lds_budget(sqt, base):
    """Wrappers over shallow leaves (height unchanged), one at a time, until the resident layout passes 160 KB: the last
    resident and the first streaming plan render bit-equal, and the last resident layout is within one wrapper of the budget."""
    bih0, cam, exp, _ = base
    nodes = bih0.nodes
    _, depth = TP.bfs_branch_numbers(nodes)
    shallow = [int(i) for i in np.nonzero((nodes["kind"] & 3) == 3)[0] if depth[i] + 2 < bih0.height]
    ps_of = lambda k: TP.PaddedScene(bih0, {i: [(0, TP.LEFT)] for i in shallow[:k]})
    assert probe(sqt, ps_of(0), cam, {})[0]["trace_form"] == "resident"
    assert probe(sqt, ps_of(len(shallow)), cam, {})[0]["trace_form"] != "resident"
    lo, hi = 0, len(shallow)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if probe(sqt, ps_of(mid), cam, {})[0]["trace_form"] == "resident":
            lo = mid
        else:
            hi = mid
    assert ps_of(hi).height == bih0.height
    last = check_frame(sqt, ps_of(lo), cam, exp, {})
    first = check_frame(sqt, ps_of(hi), cam, exp, {})
    assert last["trace_form"] == "resident" and first["trace_form"] == "streaming_six_wave"
    assert LDS - 48 < last["trace_lds_bytes"] <= LDS, last
    print(f"[limits] resident LDS: {lo} wrappers -> {last['trace_lds_bytes']} B resident, {hi} -> {first['trace_form']}")


@pytest.mark.parametrize("n_verts,form", [(4096, "resident"), (4097, "streaming_six_wave")])
def test_resident_vertex_limit(sqt, O, n_verts, form):
    """A soup of 1366 triangles with exactly 4096 / 4097 unique vertices; the triangle that adds the last vertices is large
    and in front of the camera."""
    rng = np.random.default_rng(n_verts)
    n = 1366
    c = rng.uniform(-1.5, 1.5, (n, 1, 3))
    v = (c + rng.normal(0, 0.1, (n, 3, 3))).astype(np.float32)
    v[0] = [[-2.0, -0.6, -0.6], [-2.0, 0.6, -0.4], [-2.1, 0.0, -1.2]]   # in front of the soup, facing the camera at x = -6
    v[-1] = [[-2.0, -0.6, -0.6], [-2.0, 0.65, -0.35], [-2.0, 0.0, 0.7]]
    v[-1, 0] = v[0, 0]                                                    # shares one vertex: 1365 x 3 + 2 new ones = 4097
    if n_verts == 4096:
        v[-1, 1] = v[0, 1]                                                # shares two: 4096
    mats = np.zeros(2, sqt._native.MAT_DTYPE)
    mats["surf"] = [[0.7, 0.6, 0.5], [0, 0, 0]]
    mats["emissive"] = [0, 20]
    mats["emit"] = [[0, 0, 0], [1, 1, 1]]
    tris = np.zeros(n, sqt._native.TRI_DTYPE)
    tris["v0"], tris["v1"], tris["v2"] = v[:, 0], v[:, 1], v[:, 2]
    tris["mat"] = (np.arange(n) % 9 == 0).astype(np.int32)
    assert len(np.unique(v.reshape(-1, 3).view([("x", "<f4"), ("y", "<f4"), ("z", "<f4")]))) == n_verts
    bih = sqt.BIH(sqt.Mesh.from_arrays(tris, mats))
    ob = O.BIH(_oracle_tris(O, tris, mats))
    cam_txt = b"-6 0.1 0.2\n0 0 0\n"
    cam_p, cam_o = sqt.camera_from_text(cam_txt), O.camera_from_text(cam_txt)
    last = int(np.nonzero((bih.tris["v2"] == v[-1, 2]).all(1))[0][0])
    assert last in {ob.intersect(*O.make_ray(W, H, y, x, cam_o)).tri for y in range(W) for x in range(H)}
    exp = {cast: ob.render(cam_o, 1 if cast else SPP, W, H, cast=cast, threads=THREADS)[:2] for cast in (False, True)}
    plan = check_frame(sqt, bih, cam_p, exp, {})
    assert plan["trace_form"] == form, plan
    print(f"[limits] {n_verts} unique vertices: {plan['trace_form']}")


@pytest.mark.parametrize("count,resident,packed", [(31, True, 1), (32, False, 0)])
def test_leaf_encoding_limit(sqt, O, base, count, resident, packed):
    """A leaf of 31 / 32 members beside scene.obj (_big_leaf): leaves of <= 31 triangles are packed count << 24 | first
    (resident form, streaming packed_leaves); 32 is not.  A leaf count that is truncated or mis-masked skips the last member,
    and a wrong member order picks another tie winner: both change the image (tests/test_tree_padding.py checks that)."""
    bih0, cam, _, _ = base
    cam_o = O.load_camera(os.path.join(DATA, "camera"))
    tris, mats = _big_leaf(sqt, O, bih0, cam_o, count)
    bih = sqt.BIH(sqt.Mesh.from_arrays(tris, mats))
    assert bih.longest_leaf == count
    ob = O.BIH(_oracle_tris(O, tris, mats))
    exp = {cast: ob.render(cam_o, 1 if cast else SPP, W, H, cast=cast, threads=THREADS)[:2] for cast in (False, True)}
    plan = check_frame(sqt, bih, cam, exp, {"pool": 0})           # the extra triangles make the tree 14 tall: resident only unpooled
    assert bih.height <= 14 and (plan["trace_form"] == "resident") == resident and plan["packed_leaves"] == packed, plan
    plan = check_frame(sqt, bih, cam, exp, {"resident": 0}, casts=(False,))
    assert plan["trace_form"] != "resident" and plan["packed_leaves"] == packed, plan
    print(f"[limits] leaf of {count}: {'resident' if resident else 'streaming'}, packed_leaves {packed}")


def test_streaming_tunables_on_a_tall_tree(sqt, base):
    """A height-30 padded tree under every lds_node_kb x trace_blocks_per_cu setting (only the campaign drew these)."""
    bih0, cam, exp, (axis, side) = base
    ps = TP.full_stack(bih0, 30, axis, side)
    forms = set()
    for kb in (0, 1, 4, 32, 128):
        for per_cu in (0, 1, 2, 3):
            plan = check_frame(sqt, ps, cam, exp, {"lds_node_kb": kb, "trace_blocks_per_cu": per_cu}, casts=(False,))
            assert plan["n_lds"] <= kb * 1024 // 48
            forms.add((plan["trace_form"], plan["blocks_per_cu"], plan["n_lds"] == 0))
    assert {f[0] for f in forms} == {"streaming_six_wave", "streaming_plain"} and any(f[2] for f in forms)
    print(f"[limits] tunables at height 30: {sorted(forms)}")


def test_campaign_seeds_with_streaming_tunables(sqt, O):
    """Seeds 40 000 000 .. 40 000 099 of tests/fuzz_gpu.py draw lds_node_kb and trace_blocks_per_cu."""
    import fuzz_gpu
    failures = [(seed, msg) for seed in range(40000000, 40000100) if (msg := fuzz_gpu.run_case(seed))]
    assert not failures, failures[:5]


def test_a_refused_call_touches_nothing(sqt, base):
    """A call the planner refuses for LDS (a tree one taller than the streaming form takes, on a DeviceScene of its own) between two
    renders of one 8 x 8 frame on a resident scene: the refusal has the recorded text and plan (tests/golden/plan_cases.json,
    u16_height159: nothing launched, no trace form chosen), it comes before anything is allocated, freed or cleared, and the second
    frame equals the first bit for bit."""
    import json
    bih0, cam, _, _ = base
    with open(os.path.join(GOLDEN, "plan_cases.json")) as f:
        rec = {c["name"]: c for c in json.load(f)["cases"]}["u16_height159"]
    ds, tall = sqt.DeviceScene(bih0, 0), sqt.DeviceScene(TP.full_stack(bih0, 159, 0, TP.LEFT), 0)
    try:
        first = render(ds, cam, 2, 8, 8)
        with pytest.raises(sqt.SquiglyError) as e:
            render(tall, cam, 1, 1, 1)
        assert str(e.value) == rec["refusal"] and "BIH height 159 needs" in rec["refusal"]
        plan = tall.last_plan()
        assert plan["launched"] == 0 and plan == rec["plan"]
        assert (plan["trace_form"], plan["blocks_per_cu"], plan["n_lds"], plan["trace_lds_bytes"], plan["primary_form"]) == ("per_pixel", 0, 0, 0, "none")
        assert tall.rng_table()[0] == 0 and not any(tall.stats())            # the refused scene holds no table and no workspace
        again = render(ds, cam, 2, 8, 8)
    finally:
        ds.close()
        tall.close()
    assert np.array_equal(bits(again[0]), bits(first[0])) and np.array_equal(again[1], first[1])
    assert plan["height"] == 159 and plan["stack_cap"] == 159


def test_one_shot_call_on_a_tall_tree(sqt, base):
    bih0, cam, exp, (axis, side) = base
    ps = TP.full_stack(bih0, 150, axis, side)
    a = sqt.render_f32(ps, cam, SPP, (W, H))
    assert np.array_equal(bits(a), bits(exp[False][0]))
