"""The scene packer (csrc/sq_pack_scene.h, sq_pack_scene) through its C-ABI window (sq_scene_pack, include/squigly_host.h): every
array sq_scene_upload copies to the device and every flag that chooses a kernel form, on the CPU.

* bit-equality with the commit the packer was lifted from: tests/golden/pack_digests.json holds byte counts, SHA-256 digests
  and scalars of every fixture scene as that commit's sq_scene_upload produced them;
* bit-equality of the three level-1 records (sq_pack_level1.h), which are younger than that commit, with the commit before their
  builder was rewritten: tests/golden/level1_records.json, over the fixture scenes, the named soups and a slice of fuzz_level1;
* structure, independent of that commit: the branch table decodes back to the caller's tree, the tables agree with each other;
* the material and geometry flags on both sides of their bounds; every refusal with its exact text;
* the packer under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone program (tests/pack_main.cpp).

Not covered: the 2^24-triangle switch (a scene of that size needs gigabytes and far more than a few seconds to build).
"""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import fuzz_level1 as FL
import level1_mirror_restatement as M5
import level1_restatement as R
import level1_stretch_restatement as S
import tree_padding as TP
from conftest import DATA, GOLDEN, ROOT
from scenes import ARRAYS, LEVEL1_ARRAYS, LEVEL1_SCALARS, SCALARS, big_leaf as _big_leaf, emitter_soup as _emitter_soup, pack, pack_level1

LEAF_BIT, AXIS_MASK, RUN_PAD = 0x80000000, 0x60000000, 3
BRANCH = np.dtype([("lo", "<f4", 3), ("lmax", "<f4"), ("hi", "<f4", 3), ("rmin", "<f4"), ("lmax2", "<f4"), ("rmin2", "<f4"),
                   ("left", "<u4"), ("right", "<u4")])
SQ_TEXT = b"newmtl A\nreflective 0 1 1 1\nemissive 1 1 1 1\n"


def refusal(sqt, scene_ref, out_ref=None):
    h = C.c_void_p()
    assert sqt.lib().sq_scene_pack(scene_ref, C.byref(h) if out_ref is None else out_ref) != 0
    return sqt.lib().sq_last_error().decode()


class RawScene:
    """An sq_scene over arrays given as they are (no builder): nodes as (kind, lmax, rmin, link) rows."""

    def __init__(self, sqt, nodes, tris=None, mats=None, root=((-1, -1, -1), (1, 1, 1)), height=0):
        N = sqt._native
        self.nodes = np.array(nodes, N.NODE_DTYPE)
        self.tris = np.zeros(0, N.TRI_DTYPE) if tris is None else tris
        self.mats = np.zeros(0, N.MAT_DTYPE) if mats is None else mats
        sc = self.scene = N.Scene()
        sc.root.lo[:], sc.root.hi[:] = root[0], root[1]
        sc.nodes, sc.n_nodes = self.nodes.ctypes.data, len(self.nodes)
        sc.tris, sc.n_tris = (self.tris.ctypes.data if len(self.tris) else None), len(self.tris)
        sc.mats, sc.n_mats = (self.mats.ctypes.data if len(self.mats) else None), len(self.mats)
        sc.height = height


def one_triangle(sqt, material=None, n_mats=1, v=((0, 0, 0), (1, 0, 0), (0, 1, 0)), **kw):
    """A single leaf over one triangle of material 0; material: {field: value} over a plain grey material."""
    N = sqt._native
    tris = np.zeros(1, N.TRI_DTYPE)
    tris["v0"], tris["v1"], tris["v2"] = v
    mats = np.zeros(n_mats, N.MAT_DTYPE)
    mats["surf"] = 0.5
    for k, val in (material or {}).items():
        mats[k][0] = val
    return RawScene(sqt, [(3 | (1 << 2), 0, 0, 0)], tris, mats, **kw)


def disjoint_triangles(sqt, n):
    """n triangles on a grid that share no vertex: 3 n unique vertices."""
    N = sqt._native
    i = np.arange(n)
    x, y = (i % 256).astype(np.float32), (i // 256).astype(np.float32)
    tris = np.zeros(n, N.TRI_DTYPE)
    tris["v0"] = np.stack([x, y, 0 * x], 1)
    tris["v1"] = np.stack([x + 0.5, y, 0 * x], 1)
    tris["v2"] = np.stack([x, y + 0.5, 0 * x + 0.25], 1)
    mats = np.zeros(1, N.MAT_DTYPE)
    mats["surf"] = 0.5
    return sqt.BIH(sqt.Mesh.from_arrays(tris, mats))


def fixture_scenes(sqt, O):
    """{name: object with .scene}: data/scene.obj and the smallest scenes on each side of every switch of the packer."""
    base = sqt.BIH(sqt.Mesh.from_obj(os.path.join(DATA, "scene.obj"), DATA))
    cam_o = O.load_camera(os.path.join(DATA, "camera"))
    out = {"scene_obj": base,
           "padded": TP.PaddedScene(base, TP.root_chain(5)),
           "verts_65535": disjoint_triangles(sqt, 21845), "verts_65536": disjoint_triangles(sqt, 21846),
           "empty": sqt.BIH(sqt.Mesh.from_text(b"mtllib s.sq\n", SQ_TEXT)),
           "one_branch": sqt.BIH(sqt.Mesh.from_text(b"mtllib s.sq\no X\nv -1 0 -1\nv 1 0 -1\nv 0 1 1\nusemtl A\n" + b"f 1 2 3\n" * 20, SQ_TEXT))}
    for count in (31, 32):
        out[f"leaf_{count}"] = sqt.BIH(sqt.Mesh.from_arrays(*_big_leaf(sqt, O, base, cam_o, count)))
    for seed, n_emit in ((5, 64), (6, 65)):
        out[f"emitters_{n_emit}"] = sqt.BIH(sqt.Mesh.from_arrays(*_emitter_soup(sqt, seed, n_emit)[:2]))
    return out


@pytest.fixture(scope="module")
def fixtures(sqt, O):
    return fixture_scenes(sqt, O)


@pytest.fixture(scope="module")
def packed(sqt, fixtures):
    return {name: pack(sqt, f) for name, f in fixtures.items()}


def digest_of(arrays, scalars):
    return {"arrays": {k: {"bytes": len(v), "sha256": hashlib.sha256(v).hexdigest()} for k, v in arrays.items()}, "scalars": scalars}


# ---- bit-equality with the commit the packer came from ----

def test_fixtures_sit_on_both_sides_of_every_switch(fixtures, packed):
    s = {k: v[1] for k, v in packed.items()}
    a = {k: v[0] for k, v in packed.items()}
    assert s["verts_65535"]["n_verts"] == 65535 and len(a["verts_65535"]["trix"]) > 0
    assert s["verts_65536"]["n_verts"] == 0 and len(a["verts_65536"]["trix"]) == 0 and len(a["verts_65536"]["verts4"]) == 0
    assert fixtures["leaf_31"].longest_leaf == 31 and s["leaf_31"]["packed_leaves"] == 1 and len(a["leaf_31"]["rbranch"]) > 0
    assert fixtures["leaf_32"].longest_leaf == 32 and s["leaf_32"]["packed_leaves"] == 0 and len(a["leaf_32"]["rbranch"]) == 0
    assert len(a["leaf_32"]["trix"]) == 0 and s["leaf_32"]["n_verts"] > 0      # the vertices stay, the index form goes
    assert s["emitters_64"]["n_emitters"] == 64 and s["emitters_65"]["n_emitters"] == -1 and len(a["emitters_65"]["emitters"]) == 65 * 4
    assert (s["empty"]["n_branches"], s["empty"]["n_leaves"], len(a["empty"]["tris"])) == (0, 1, RUN_PAD * 36)
    assert s["empty"]["cull_o2max"] == np.float32(-1).view(np.uint32) and a["empty"]["cull_child"] == b""
    assert (s["one_branch"]["n_branches"], s["one_branch"]["n_leaves"], s["one_branch"]["height"]) == (1, 2, 2)


def test_packed_bytes_equal_the_recorded_ones(packed):
    """Every array (byte count, SHA-256) and every scalar of every fixture scene is what the recorded commit's
    sq_scene_upload built (the JSON says which commit and how)."""
    golden = json.load(open(os.path.join(GOLDEN, "pack_digests.json")))
    assert golden["commit"].startswith("d305fd1")
    assert set(golden["scenes"]) == set(packed)
    for name, (arrays, scalars) in packed.items():
        got, want = digest_of(arrays, scalars), golden["scenes"][name]
        assert set(want["arrays"]) == set(ARRAYS) and set(want["scalars"]) == set(SCALARS)
        for k in ARRAYS:
            assert got["arrays"][k] == want["arrays"][k], (name, k)
        assert got["scalars"] == want["scalars"], name


# ---- the level-1 records: bit-equality with the commit before their builder was written once ----
LEVEL1_FUZZ_SEEDS = tuple(range(3000, 3200))             # the pytest slice of tests/fuzz_level1.py: every EDGES scene at least twice


def parallel_quads(n):
    """fuzz_level1's "groups13" with n parallel mirror quads: more thin (axis, cell) groups than the cover's grouping keeps (56), which
    no family of fuzz_level1 reaches -- a lattice has at most 15 planes, a soup 13 quads."""
    q = [(M5.quad((-1.5, -1.5, -2.0 + 0.07 * k), (3, 0, 0), (0, 3, 0)), 1 + k % 2) for k in range(n)]
    return M5.mirror_soup(57, 1, q, cluster=(1.2, 1.2, 2.6), emitter_size=0.5)


def level1_scenes(sqt, fixtures):
    """{name: object with .scene} of tests/golden/level1_records.json: the fixture scenes, the named soups of the level-1 tests and
    fuzz_level1.case(seed) of LEVEL1_FUZZ_SEEDS, an edge scene with its edge in the name."""
    out = dict(fixtures)
    for name, make in R.NAMED_SOUPS.items():
        out[name] = sqt.BIH(sqt.Mesh.from_arrays(*make()[:2]))
    for name, make in (("axis_soup", M5.axis_soup), ("tilted_soup", M5.tilted_soup)):
        out[name] = sqt.BIH(sqt.Mesh.from_arrays(*make()[0][:2]))
    out["parallel_57"] = sqt.BIH(sqt.Mesh.from_arrays(*parallel_quads(57)[:2]))
    for seed in LEVEL1_FUZZ_SEEDS:
        c = FL.case(seed)
        out[f"fuzz_{seed}" + (f"_{c.edge}" if c.edge else "")] = FL.product_bih(c)
    return out


@pytest.fixture(scope="module")
def level1_packed(sqt, fixtures):
    return {name: pack_level1(sqt, f) for name, f in level1_scenes(sqt, fixtures).items()}


def test_level1_records_equal_the_recorded_ones(level1_packed):
    """Arrays "level1", "level1_cover" and "level1_mirror" (byte count, SHA-256) and the scalars level1_on, level1_zero and
    shortcut_depth of every scene are what the recorded commit's packer built (the JSON says which commit and how).  No scene is
    skipped: a record that a cap turned off is pinned as it is."""
    golden = json.load(open(os.path.join(GOLDEN, "level1_records.json")))
    assert golden["commit"].startswith("092ca5d")
    assert set(golden["scenes"]) == set(level1_packed)
    for name, (arrays, scalars) in level1_packed.items():
        got, want = digest_of(arrays, scalars), golden["scenes"][name]
        assert set(want["arrays"]) == set(LEVEL1_ARRAYS) and set(want["scalars"]) == set(LEVEL1_SCALARS)
        for k in LEVEL1_ARRAYS:
            assert got["arrays"][k] == want["arrays"][k], (name, k)
        assert got["scalars"] == want["scalars"], name


def test_level1_scenes_sit_on_both_sides_of_every_switch(level1_packed):
    """From the records alone: the recorded scenes hold both values of everything the builder of the three records branches on and
    a record can show.  (What a record cannot show -- a merge loop that ran, the 56-group overflow -- was counted once at the
    recorded commit: DESIGN.md 4.1, "Host side split by role".)"""
    T, V, M, on = {}, {}, {}, {}
    for name, (a, s) in level1_packed.items():
        T[name] = np.frombuffer(a["level1"], R.LEVEL1)[0]
        V[name] = np.frombuffer(a["level1_cover"], S.COVER)[0] if a["level1_cover"] else None
        M[name] = np.frombuffer(a["level1_mirror"], M5.MIRROR)[0] if a["level1_mirror"] else None
        on[name] = s["level1_on"]
        assert on[name] == T[name]["on"] and (V[name] is None) == (M[name] is None), name
    edge = lambda e: [n for n in level1_packed if n.startswith("fuzz_") and n.endswith("_" + e)]
    assert set(on.values()) == {0, 1}
    assert {int(T[n]["n_classes"]) for n in T if on[n]} == {1, 2, 3, 4}
    covers = {int(V[n]["n"]) for n in V if V[n] is not None}
    assert 8 in covers and min(covers) < 8
    assert any(on[n] and V[n] is None for n in V)                             # on, and no cover at all
    assert all(V[n] is None for n in V if not on[n])
    for e, field, n in (("groups12", "n_panels", 12), ("w8", "n_w", 8)):      # at a cap: the record holds as many as fit
        assert len(edge(e)) >= 2 and all(M[x] is not None and M[x]["n_panels"] > 0 and M[x][field] == n for x in edge(e)), e
    for e in ("groups13", "w9"):                                              # one more: a cover, and condition (5) off
        assert len(edge(e)) >= 2 and all(on[x] and M[x] is not None and M[x]["n_panels"] == 0 for x in edge(e)), e
    assert {int(M[n]["n_rest"]) for n in M if M[n] is not None and M[n]["n_panels"] > 0} >= {0, 1, 4}
    for e_on, e_off in (("emit64", "emit65"), ("P_under", "P_over")):
        assert len(edge(e_on)) >= 2 and len(edge(e_off)) >= 2
        assert all(on[x] for x in edge(e_on)) and not any(on[x] for x in edge(e_off)), (e_on, e_off)


@pytest.mark.parametrize("n_mats,fits", [(65535, True), (65536, False)])
def test_material_count_switch(sqt, n_mats, fits):
    """The 16-bit material index of a trix record: 65535 materials fit, 65536 do not (too large for a recorded fixture)."""
    arrays, scalars = pack(sqt, one_triangle(sqt, n_mats=n_mats))
    assert (len(arrays["trix"]) == 8) == fits and (scalars["n_verts"] == 3) == fits and len(arrays["mats"]) == 32 * n_mats


# ---- structure ----

def decode_tree(branches, leaves, scalars):
    """The pre-order sq_node rows the branch table stands for, and the branch number at each pre-order position (-1: leaf)."""
    rows, number = [], []
    todo = [("visit", scalars["root_ref"])]
    while todo:
        what, x = todo.pop()
        if what == "link":                                 # the left subtree of rows[x] is complete: its right child comes next
            rows[x][3] = len(rows)
            continue
        if x & LEAF_BIT:
            first, count = ((x & 0xFFFFFF, (x >> 24) & 31) if scalars["packed_leaves"] else
                            (int(leaves[x & ~LEAF_BIT][0]), int(leaves[x & ~LEAF_BIT][1])))
            rows.append([3 | (count << 2), np.float32(0), np.float32(0), first]); number.append(-1)
            continue
        b = branches[x]
        rows.append([(int(b["left"]) >> 29) & 3, b["lmax"], b["rmin"], -1]); number.append(x)
        todo += [("visit", int(b["right"])), ("link", len(rows) - 1), ("visit", int(b["left"]) & ~AXIS_MASK)]
    return rows, np.array(number)


@pytest.mark.parametrize("name", ["scene_obj", "padded"])
def test_tables_decode_to_the_tree_and_agree_with_each_other(sqt, fixtures, packed, name):
    nodes = fixtures[name].nodes
    arrays, s = packed[name]
    branches = np.frombuffer(arrays["branches"], BRANCH)
    leaves = np.frombuffer(arrays["leaves"], "<i4").reshape(-1, 2)
    nb = s["n_branches"]
    assert len(branches) == nb and len(leaves) == s["n_leaves"] and nb + s["n_leaves"] == len(nodes)
    rows, number = decode_tree(branches, leaves, s)
    assert len(rows) == len(nodes)
    for field, col in (("kind", 0), ("lmax", 1), ("rmin", 2), ("link", 3)):
        want = nodes[field]
        got = np.array([r[col] for r in rows], want.dtype)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), field
    num, _ = TP.bfs_branch_numbers(nodes)                  # breadth-first, stable within a level
    assert np.array_equal(number, num)
    assert np.array_equal(branches["lmax2"].view(np.uint32), branches["lmax"].view(np.uint32))
    assert np.array_equal(branches["rmin2"].view(np.uint32), branches["rmin"].view(np.uint32))
    words = np.frombuffer(arrays["branches"], "<u4").reshape(nb, 12)
    # rbranch: lo, lmax | hi, rmin | left word, right word (whose bits 30..29 are its own: the grown children)
    rb = np.frombuffer(arrays["rbranch"], "<u4").reshape(nb, 10)
    assert s["packed_leaves"] == 1
    assert np.array_equal(rb[:, :8], words[:, :8]) and np.array_equal(rb[:, 8], words[:, 10])
    assert np.array_equal(rb[:, 9] & ~np.uint32(AXIS_MASK), words[:, 11])
    # branches_m: the branch record, then the binary16 culling boxes of its children
    bm = np.frombuffer(arrays["branches_m"], "<u4").reshape(nb, 20)
    c16 = np.frombuffer(arrays["cull_child16"], "<u4").reshape(nb, 8)
    assert np.array_equal(bm[:, :12], words) and np.array_equal(bm[:, 12:], c16)
    # cull_child16 is sq_half_outward of cull_child: lo down, hi up, the fourth word of a box unused
    cc = np.frombuffer(arrays["cull_child"], "<f4").reshape(nb, 2, 2, 4)
    half = sqt.lib().sq_half_outward
    want16 = np.zeros((nb, 2, 4), np.uint32)
    for b in range(nb):
        for side in range(2):
            for c in range(3):
                want16[b, side, c] = half(float(cc[b, side, 0, c]), 0) | (half(float(cc[b, side, 1, c]), 1) << 16)
    assert np.array_equal(c16.reshape(nb, 2, 4), want16) and not cc[..., 3].any()
    boxes, limits = (fixtures[name].cull_boxes() if name == "padded" else (None, None))
    if boxes is not None:                                  # ... and cull_child is sq_cull_boxes of the two children, by branch number
        br = np.nonzero(num >= 0)[0]
        assert np.array_equal(cc[num[br], 0, :, :3].reshape(-1, 6), boxes[br + 1])
        assert np.array_equal(cc[num[br], 1, :, :3].reshape(-1, 6), boxes[nodes["link"][br]])
        assert np.float32(limits[0]).view(np.uint32) == s["cull_o2max"]
    n_tris = fixtures[name].scene.n_tris
    assert len(arrays["tris"]) == (n_tris + RUN_PAD) * 36 and not any(arrays["tris"][n_tris * 36:])
    assert len(arrays["trix"]) == n_tris * 8


def test_resident_tables_come_and_go_together(packed):
    """trix, rbranch and rroot are the resident encoding: all there or all absent.  (rroot alone cannot say which: it is the
    root's reference, and a root that is a branch has number 0.)"""
    for name, (arrays, s) in packed.items():
        assert (len(arrays["trix"]) == 0) == (len(arrays["rbranch"]) == 0) or s["n_branches"] == 0, name
        if len(arrays["trix"]) == 0:
            assert s["rroot"] == 0, name
        if s["rroot"] != 0:
            assert len(arrays["trix"]) > 0 and s["rroot"] & LEAF_BIT, name
        assert len(arrays["tris"]) % 36 == 0 and not any(arrays["tris"][-RUN_PAD * 36:]), name


# ---- flags ----

def test_material_values_that_clear_nonneg_materials(sqt):
    flag = lambda **m: pack(sqt, one_triangle(sqt, m))[1]["nonneg_materials"]
    assert flag() == 1
    assert flag(reflective=-0.0) == 0 and flag(surf=(0.5, -0.0, 0.5)) == 0
    assert flag(emissive=np.nan) == 0 and flag(surf=(0.5, 0.5, np.nan)) == 0
    assert flag(surf=(3.1e38, 0, 0)) == 0 and flag(surf=(3.0e38, 0, 0)) == 1
    assert flag(emissive=1e30, emit=(1e30, 0, 0)) == 0                       # every component finite, the product inf
    # max_s * max_e + max_e against 3e38, with max_s = 1: 2 * 1.49e38 is below, 2 * 1.51e38 above; every component <= 3e38
    assert flag(surf=(1, 0, 0), emissive=1.0, emit=(1.49e38, 0, 0)) == 1
    assert flag(surf=(1, 0, 0), emissive=1.0, emit=(1.51e38, 0, 0)) == 0
    assert flag(surf=(0, 0, 0), emissive=1.0, emit=(2.9e38, 0, 0)) == 1      # the same bound with max_s = 0


def shortcut_depth(sqt, holder):
    """The packer's shortcut_depth (not among SCALARS: the recorded digests are older than it)."""
    L, h, v = sqt.lib(), C.c_void_p(), C.c_int64()
    sqt._native.check(L.sq_scene_pack(C.byref(holder.scene), C.byref(h)))
    try:
        assert L.sq_packed_scalar(h, b"shortcut_depth", C.byref(v)) == 0
    finally:
        L.sq_packed_free(h)
    return v.value


def test_shortcut_depth_is_the_deepest_path_whose_nested_products_stay_finite(sqt):
    """nonneg_materials bounds one product, the reference's depth 3.  A path of depth D nests D - 2, and the s == 0 shortcuts of the
    generic-depth kernels stay exact while max_e * (1 + max_s + ... + max_s^(D-2)) <= 3e38: shortcut_depth is the largest such D
    up to 8, at least 3 where nonneg_materials holds, 0 where it does not.  The expected value is that sum in exact rationals."""
    from fractions import Fraction
    depth = lambda **m: shortcut_depth(sqt, one_triangle(sqt, m))
    assert depth() == 8                                                       # no emission: nothing to overflow
    assert depth(surf=(0.5, -0.0, 0.5)) == 0 and depth(emissive=np.nan) == 0  # nonneg_materials off
    assert depth(surf=(1, 0, 0), emissive=1.0, emit=(1.51e38, 0, 0)) == 0     # ... by its own bound
    assert depth(surf=(1, 0, 0), emissive=1.0, emit=(1.49e38, 0, 0)) == 3     # 2 e <= 3e38 < 3 e
    assert depth(surf=(1, 0, 0), emissive=1.0, emit=(4.4e37, 0, 0)) == 7      # 6 e <= 3e38 < 7 e
    assert depth(surf=(1, 0, 0), emissive=1.0, emit=(3.7e37, 0, 0)) == 8      # 7 e <= 3e38
    assert depth(surf=(1e10, 0, 0), emissive=1.0, emit=(1e18, 0, 0)) == 4     # 1e18 * 1e20 fits, 1e18 * 1e30 does not
    assert depth(surf=(3e38, 3e38, 3e38), emissive=1e-3, emit=(1, 0, 0)) == 3 # every power stays finite in double
    assert depth(surf=(3e38, 0, 0), emissive=0.0, emit=(3e38, 0, 0)) == 8
    for s in (0.0, 0.5, 1.0, 2.0, 1e5, 1e10, 1e19, 3e38):
        for e in (0.0, 1e-30, 1.0, 1e10, 1e20, 1e30, 1e37, 2.9e38):
            fs, fe = Fraction(float(np.float32(s))), Fraction(float(np.float32(e)))
            holds = [D for D in range(3, 9) if fe * sum(fs ** i for i in range(D - 1)) <= Fraction(3.0e38)]
            want = 0
            for D in range(3, 9):                                             # the bound grows with D: the first failure ends it
                if D not in holds:
                    break
                want = D
            holder = one_triangle(sqt, dict(surf=(s, 0, 0), emissive=1.0, emit=(e, 0, 0)))
            assert shortcut_depth(sqt, holder) == want, (s, e)
            assert pack(sqt, holder)[1]["nonneg_materials"] == (want >= 3), (s, e)


def test_geometry_values_that_clear_finite_geometry(sqt):
    assert pack(sqt, one_triangle(sqt))[1]["finite_geometry"] == 1
    assert pack(sqt, one_triangle(sqt, v=((0, 0, 0), (1, np.nan, 0), (0, 1, 0))))[1]["finite_geometry"] == 0
    assert pack(sqt, one_triangle(sqt, root=((-1, -1, -1), (1, np.inf, 1))))[1]["finite_geometry"] == 0
    leaf = (3, 0, 0, 0)
    assert pack(sqt, RawScene(sqt, [(0, 0.5, -0.5, 2), leaf, leaf]))[1]["finite_geometry"] == 1
    assert pack(sqt, RawScene(sqt, [(0, np.inf, -0.5, 2), leaf, leaf]))[1]["finite_geometry"] == 0


def test_emitter_list_and_its_off_switch(sqt):
    n = lambda **m: pack(sqt, one_triangle(sqt, m))[1]["n_emitters"]
    assert n() == 0 and n(emissive=2.0, emit=(1, 0, 0)) == 1
    assert n(emissive=2.0, emit=(-0.0, 0, 0)) == 1                           # not exactly +0
    assert n(emissive=np.inf, emit=(1, 1, 1)) == -1 and n(surf=(np.nan, 0, 0)) == -1


# ---- refusals ----

LEAF1 = (3 | (1 << 2), 0, 0, 0)


def test_argument_refusals(sqt):
    N = sqt._native
    good = one_triangle(sqt)
    assert refusal(sqt, None) == "null argument"
    assert refusal(sqt, C.byref(good.scene), out_ref=C.POINTER(C.c_void_p)()) == "null argument"
    sc = one_triangle(sqt); sc.scene.nodes = None
    assert refusal(sqt, C.byref(sc.scene)) == "scene has no nodes"
    sc = one_triangle(sqt); sc.scene.n_nodes = 0
    assert refusal(sqt, C.byref(sc.scene)) == "scene has no nodes"
    for field, value in (("n_tris", -1), ("n_mats", -1), ("tris", None), ("mats", None)):
        sc = one_triangle(sqt); setattr(sc.scene, field, value)
        assert refusal(sqt, C.byref(sc.scene)) == "bad triangle/material arrays", field
    for mat in (1, -1):
        sc = one_triangle(sqt); sc.tris["mat"][0] = mat
        assert refusal(sqt, C.byref(sc.scene)) == f"triangle 0: material {mat} outside 0..0"
    assert N.lib().sq_last_error() != b""


def test_tree_refusals(sqt):
    """Every message validate_tree can give (its "scene has no nodes" and "not in pre-order position" cannot be reached:
    the argument check and the link check come first) and the height check."""
    leaf0 = (3, 0, 0, 0)
    tri = one_triangle(sqt)
    cases = [([(3 | (2 << 2), 0, 0, 0)], "leaf 0 has triangle range [0,+2) outside 0..1"),
             ([(3 | (1 << 2), 0, 0, 1)], "leaf 0 has triangle range [1,+1) outside 0..1"),
             ([(3, 0, 0, -1)], "leaf 0 has triangle range [-1,+0) outside 0..1"),
             ([(3 | (-1 << 2), 0, 0, 0)], "leaf 0 has triangle range [0,+-1) outside 0..1"),
             ([(1 | (1 << 2), 0, 0, 2), leaf0, leaf0], "branch 0 has stray bits in kind"),
             ([(0, 0, 0, 1)], "branch 0 has no left child"),
             ([(0, 0, 0, 2), leaf0, (1, 0, 0, 4)], "branch 2 has no left child"),
             ([(0, 0, 0, 1), leaf0, leaf0], "branch 0: right child link 1, expected 2"),
             ([(0, 0, 0, 3), leaf0, leaf0], "branch 0: right child link 3, expected 2"),
             ([(0, 0, 0, 2), leaf0], "branch 0: right child 2 out of range"),
             ([leaf0, leaf0], "tree covers 1 of 2 nodes"),
             ([(0, 0, 0, 2), leaf0, leaf0, leaf0], "tree covers 3 of 4 nodes")]
    for nodes, message in cases:
        sc = RawScene(sqt, nodes, tri.tris, tri.mats)
        assert refusal(sqt, C.byref(sc.scene)) == message, nodes
    sc = RawScene(sqt, [(0, 0, 0, 2), leaf0, leaf0], tri.tris, tri.mats, height=3)
    assert refusal(sqt, C.byref(sc.scene)) == "scene.height = 3 but the tree has height 2"
    sc.scene.height = 2
    assert pack(sqt, sc)[1]["height"] == 2


def test_upload_checks_the_device_before_the_tree(sqt):
    """sq_scene_upload: the argument and material checks, then the device, then the packer.  Without a device a malformed
    tree still reports the missing device, and a bad material index is reported before that."""
    def upload_error(sc):
        h = C.c_void_p()
        assert sqt.lib().sq_scene_upload(C.byref(sc.scene), 0, C.byref(h)) != 0
        return sqt.lib().sq_last_error().decode()
    tri = one_triangle(sqt)
    malformed = RawScene(sqt, [(3, 0, 0, 0), (3, 0, 0, 0)], tri.tris, tri.mats)
    both = RawScene(sqt, [(3, 0, 0, 0), (3, 0, 0, 0)], tri.tris.copy(), tri.mats)
    both.tris["mat"][0] = 5
    assert upload_error(both) == "triangle 0: material 5 outside 0..0"
    if sqt.device_count() == 0:
        assert upload_error(malformed) == "no HIP device available (this library has no CPU fallback)"
    else:
        assert upload_error(malformed) == "tree covers 1 of 2 nodes"


# ---- sanitizers ----

def test_packer_under_address_and_undefined_behaviour_sanitizers(sqt, tmp_path):
    """tests/pack_main.cpp (its own main: load data/scene.obj, build, pack, read every array through the window, plan a handful of
    calls through sq_plan_call, free; then the same without the plans for every raw scene file) compiled with sq_host.cpp under
    -fsanitize=address,undefined and run as a child process, once: exit 0, nothing on stderr.  The raw scene files are the edge scenes
    of the recorded slice, fuzz_level1's seeds 3000 .. 3067 with seed % 4 == 3 -- each of EDGES once --, so that every early return of
    the level-1 builder runs under the sanitizers."""
    exe = str(tmp_path / "pack_main")
    csrc = os.path.join(ROOT, "squigly-trace_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-static-libasan", "-static-libubsan",      # the runtimes inside the program: nothing to order at load time
                           os.path.join(csrc, "sq_host.cpp"), os.path.join(ROOT, "tests", "pack_main.cpp"), "-o", exe])
    files = []
    for seed in range(3003, 3068, 4):
        c = FL.case(seed)
        tris = np.zeros(len(c.v), sqt._native.TRI_DTYPE)
        tris["v0"], tris["v1"], tris["v2"], tris["mat"] = c.v[:, 0], c.v[:, 1], c.v[:, 2], c.mat
        files.append(str(tmp_path / f"fuzz_{seed}_{c.edge}.raw"))
        with open(files[-1], "wb") as f:
            f.write(np.array([len(tris), len(c.mats)], "<i4").tobytes() + tris.tobytes() + c.mats.tobytes())
    assert len(files) == len(FL.EDGES)
    r = subprocess.run([exe, os.path.join(DATA, "scene.obj"), DATA] + files, capture_output=True)
    assert r.returncode == 0 and r.stderr == b"", (r.returncode, r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert len(lines) == 1 + len(files) and all(line.startswith(b"packed 16 arrays") for line in lines), r.stdout
    assert b"planned 10 calls" in lines[0]
