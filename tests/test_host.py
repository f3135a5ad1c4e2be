"""CPU tests of the product's host side (loaders, BIH build/flatten, C-ABI surface) against the oracle."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import library_surface as LS
from conftest import DATA, ROOT


def test_library_exports_every_declared_symbol(sqt):
    """Every function declared in include/*.h is exported by libsquigly_hip.so (no compute calls)."""
    LS.check_exports(sqt, ("squigly_hip.h", "squigly_host.h"), "sq_", exact=False)
    assert sqt.lib().sq_abi_version() == 1


def test_loader_matches_oracle(sqt, O, product_scene, oracle_scene):
    _, _, mesh = product_scene
    _, _, otris = oracle_scene
    t = mesh.tris
    assert len(t) == len(otris) == 6238
    assert np.array_equal(t["v0"], otris["a"]) and np.array_equal(t["v1"], otris["b"]) and np.array_equal(t["v2"], otris["c"])
    mats = mesh.materials
    assert np.array_equal(mats["reflective"][t["mat"]], otris["reflective"])
    assert np.array_equal(mats["surf"][t["mat"]], otris["surf"])
    assert np.array_equal(mats["emissive"][t["mat"]], otris["emissive"]) and np.array_equal(mats["emit"][t["mat"]], otris["emit"])


def test_bih_build_matches_oracle_tree(sqt, O, product_scene, oracle_scene):
    bih, cam, _ = product_scene
    ob, ocam, _ = oracle_scene
    assert (bih.height, bih.num_leaves, bih.longest_leaf) == (ob.height, ob.num_leaves, ob.longest_leaf) == (13, 640, 14)
    kind, lmax, rmin, cnt = ob.preorder()
    nd = bih.nodes
    assert np.array_equal(nd["kind"] & 3, kind)
    br = kind != 3
    assert np.array_equal(nd["lmax"][br], lmax[br]) and np.array_equal(nd["rmin"][br], rmin[br])
    assert np.array_equal((nd["kind"] >> 2)[~br], cnt[~br])
    flat = ob.flatten()
    pt = bih.tris
    assert np.array_equal(pt["v0"], flat["a"]) and np.array_equal(pt["v1"], flat["b"]) and np.array_equal(pt["v2"], flat["c"])
    assert np.array_equal(bih.bounds, ob.bounds())
    # leaves index the flattened triangles contiguously, in order
    firsts = nd["link"][~br]
    assert firsts[0] == 0 and np.array_equal(firsts[1:], np.cumsum(cnt[~br])[:-1])
    assert np.array_equal(np.array(list(cam.rot), np.float32), O.camera_arrays(ocam)[1])
    assert list(cam.pos) == [0.0, 7.0, 0.75]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_bih_build_random_soups_match_oracle(sqt, O, seed):
    """Random triangle soups incl. duplicates (equal centroids -> empty sides) and ragged sizes."""
    rng = np.random.default_rng(seed)
    n = [14, 15, 400][seed]
    v = rng.uniform(-3, 3, (n, 3, 3)).astype(np.float32)
    if seed == 2:
        v[50:90] = v[50]                       # 40 identical triangles
        v[:, :, 2] = np.round(v[:, :, 2])      # many exactly-equal coordinates: exercises longest-axis ties
    tris = np.zeros(n, sqt._native.TRI_DTYPE)
    tris["v0"], tris["v1"], tris["v2"] = v[:, 0], v[:, 1], v[:, 2]
    mats = np.zeros(1, sqt._native.MAT_DTYPE)
    bih = sqt.BIH(sqt.Mesh.from_arrays(tris, mats))
    ot = np.zeros(n, O.TRI_DTYPE)
    ot["a"], ot["b"], ot["c"] = v[:, 0], v[:, 1], v[:, 2]
    ob = O.BIH(ot)
    kind, lmax, rmin, cnt = ob.preorder()
    nd = bih.nodes
    assert len(nd) == len(kind) and np.array_equal(nd["kind"] & 3, kind)
    br = kind != 3
    assert np.array_equal(nd["lmax"][br], lmax[br]) and np.array_equal(nd["rmin"][br], rmin[br])
    assert np.array_equal((nd["kind"] >> 2)[~br], cnt[~br])
    assert np.array_equal(bih.tris["v0"], ob.flatten()["a"])
    assert (bih.height, bih.num_leaves, bih.longest_leaf) == (ob.height, ob.num_leaves, ob.longest_leaf)


def test_loader_edge_cases_match_oracle(sqt, O):
    sq = b"newmtl A\nreflective 0 1 1 1\nemissive 0 0 0 0\n\nnewmtl B\nreflective 1 0.5 0.5 0.5\nemissive 2 1 1 1\n"
    obj = (b"mtllib s.sq\r\no Cube.001_x\r\nv 0 0 0\r\nv 1 0 0\r\nv 0 1 0\r\nusemtl A\r\ns off\r\nf 1 2 3\r\n"
           b"o Second\nv 0 0 1\nusemtl B\ns on\nf 1 2 4\nf 4 2 1\n")
    cases = [(obj, sq), (obj.replace(b"usemtl B", b"usemtl C"), sq),
             (obj, sq + b"newmtl A\nreflective 0 0 0 0\nemissive 0 0 0 0\n"), (b"mtllib s.sq\n", sq),
             (obj, b" " + sq)]           # leading blank: `many loadMtl` stops at once -> no materials -> no triangles
    for o, s in cases:
        pt, ot = sqt.Mesh.from_text(o, s), O.tris_from_text(o, s)
        assert len(pt) == len(ot)
        if len(ot):
            t, m = pt.tris, pt.materials
            assert np.array_equal(t["v0"], ot["a"]) and np.array_equal(t["v2"], ot["c"])
            assert np.array_equal(m["reflective"][t["mat"]], ot["reflective"]) and np.array_equal(m["emit"][t["mat"]], ot["emit"])
    bad = [b"o X\n", b"mtllib s.sq\no X\nv 0 0 0\nf 1 1 1\n", b"mtllib s.sq\no X\nv 0 0 0\nusemtl A\nf 1/1 1 1\n",
           b"mtllib s.sq\no X\nv 0 0 0\nusemtl A\nf 1 1 2\n", b"mtllib s.sq\no X\nv 1e-3 0 0\nusemtl A\nf 1 1 1\n",
           b"mtllib s.sq\no X\nv .5 0 0\nusemtl A\nf 1 1 1\n", b"mtllib s.sq\no X\nv 0 0 0\nusemtl A\ns 1\nf 1 1 1\n",
           b"mtllib s.sq\no X\nv 0 0 0\nusemtl A\nf 0 1 1\n"]
    for o in bad:
        with pytest.raises(sqt.SquiglyError):
            sqt.Mesh.from_text(o, sq)
        with pytest.raises(O.OracleError):
            O.tris_from_text(o, sq)
    with pytest.raises(sqt.SquiglyError):
        sqt.Mesh.from_obj("/nonexistent.obj", DATA)
    with pytest.raises(sqt.SquiglyError):
        sqt.camera_from_text(b"0 7\n")
    # the last three: angles whose quadrant count leaves the range of long long (the range reduction's integer conversion
    # was undefined there; found by the ASan/UBSan build of the host side, tools/sanitize_host.sh) -- defined now, and the same bits on both sides (the two-term reduction is only accurate for moderate angles: that is the numeric spec)
    for ang in [(0.3, -1.2, 2.5), (0, 0, 0), (1.5707963267948966, 0, -0.09817477042468103), (100.0, -37.5, 6.25),
                (6.4631e21, 0.5, -1.0), (-3.0e30, 1.0e19, 7.3e18), (3.4e38, -3.4e38, 2.0 ** 63)]:
        r = (C.c_float * 9)()
        O.lib().sqo_rot_matrix_rads(*ang, O.TRIG_CRD, r)
        got = sqt.rot_matrix_rads(*ang).ravel()
        assert np.array_equal(got.view(np.uint32), np.array(list(r), np.float32).view(np.uint32))


def test_render_without_gpu_fails_loudly_not_silently(sqt, product_scene):
    """No CPU fallback: without a HIP device the render entry point returns an error."""
    if sqt.device_count() > 0:
        pytest.skip("a GPU is present")
    bih, cam, mesh = product_scene
    with pytest.raises(sqt.SquiglyError, match="no HIP device|no CPU fallback"):
        sqt.render_rgb8(bih, cam, 1, (4, 4))
    with pytest.raises(sqt.SquiglyError, match="no HIP device"):
        sqt.BIH(mesh, device=0)                      # the GPU build does not quietly become the host build


def test_shard_helpers(sqt):
    from importlib import import_module
    d = import_module("squigly-trace_amd.dist")
    L = sqt.lib()
    for w, rb, world in [(1920, 8, 8), (1080, 8, 4), (37, 8, 3), (5, 8, 2), (64, 1, 64), (100, 16, 1)]:
        seen = []
        for r in range(world):
            sh = sqt.Shard(rb, r, world)
            rows = d.shard_rows(w, rb, r, world)
            assert L.sq_shard_rows(w, sh) == len(rows)
            assert [L.sq_shard_global_row(j, sh) for j in range(len(rows))] == rows
            seen += rows
        assert sorted(seen) == list(range(w))
    assert L.sq_shard_rows(10, sqt.Shard(0, 0, 1)) == -1 and L.sq_shard_rows(10, sqt.Shard(4, 2, 2)) == -1


def test_product_does_not_touch_the_oracle():
    """The product path may not import, link or call anything under oracle/."""
    pkg = os.path.join(ROOT, "squigly-trace_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".h", ".hip", ".cpp")):
                text = open(os.path.join(dp, f), errors="replace").read()
                assert "pyoracle" not in text and "sqo_" not in text and "sq_oracle" not in text, os.path.join(dp, f)
                assert "/root/reference" not in text
    ldd = subprocess.check_output(["ldd", os.path.join(pkg, "libsquigly_hip.so")]).decode()
    assert "oracle" not in ldd
    # the measurement aids under tools/ stay away from it too: checker scripts live under tests/
    for f in os.listdir(os.path.join(ROOT, "tools")):
        if f.endswith((".py", ".sh")):
            text = open(os.path.join(ROOT, "tools", f), errors="replace").read()
            assert "pyoracle" not in text and "sqo_" not in text, f


def test_hit_distance_is_monotone_in_t():
    """The trace kernel compares two hits of one ray by t first and evaluates dist = norm((o + t*d) - o) only when
    t does not decide (csrc/sq_scene.h: dist_gt).  That rests on dist being monotone non-decreasing in t under
    round-to-nearest fp32; check it on adjacent and random t pairs, including tiny, huge and mixed-sign inputs."""
    rng = np.random.default_rng(3)
    f = np.float32

    def dist(o, d, t):
        p = o + t[:, None] * d
        v = p - o
        return np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2], dtype=np.float32)

    n = 400000
    scale = (10.0 ** rng.uniform(-6, 6, (n, 1))).astype(f)
    o = (rng.normal(size=(n, 3)) * scale).astype(f)
    d = (rng.normal(size=(n, 3)) * (10.0 ** rng.uniform(-3, 3, (n, 1)))).astype(f)
    d[rng.random(n) < 0.1, 0] = 0
    d[rng.random(n) < 0.1, 1] = -0.0
    t1 = (10.0 ** rng.uniform(-4, 4, n)).astype(f)
    for t2 in (np.nextafter(t1, f(np.inf)), (t1 * (1 + 10.0 ** rng.uniform(-7, 0, n))).astype(f), (t1 + f(1e-4)).astype(f)):
        with np.errstate(over="ignore", invalid="ignore"):
            d1, d2 = dist(o, d, t1), dist(o, d, t2.astype(f))
        assert np.all(t2 >= t1)
        assert np.all(d2 >= d1), int((d2 < d1).sum())


def test_loader_differential_fuzz_slice(sqt, O):
    """A slice of tests/fuzz_loader.py: random .obj / .sq / camera texts from the reference grammar plus byte
    mutations; the product loader and the oracle's accept and reject the same inputs and agree bit for bit."""
    import fuzz_loader
    failures = [(seed, msg) for seed in range(5000, 7000) if (msg := fuzz_loader.run_case(seed))]
    assert not failures, failures[:3]


def test_bih_build_matches_oracle_on_fuzz_scenes(sqt, O):
    """The host BIH build against the oracle's tree on the scene generators of tests/fuzz_gpu.py (ties, duplicates,
    slivers, overflowing magnitudes, NaN / infinite coordinates, long identical-triangle leaves): every node and the
    leaf order, bit for bit."""
    import fuzz_gpu as F
    for seed in range(3000, 3400):
        rng = np.random.default_rng(seed)
        v, mats, mat, _ = F.make_scene(rng)
        tris = np.zeros(len(v), sqt._native.TRI_DTYPE)
        tris["v0"], tris["v1"], tris["v2"], tris["mat"] = v[:, 0], v[:, 1], v[:, 2], mat
        bih = sqt.BIH(sqt.Mesh.from_arrays(tris, mats))
        ot = np.zeros(len(v), O.TRI_DTYPE)
        ot["a"], ot["b"], ot["c"] = v[:, 0], v[:, 1], v[:, 2]
        for f in ("reflective", "surf", "emissive", "emit"):
            ot[f] = mats[f][mat]
        ob = O.BIH(ot)
        kind, lmax, rmin, cnt = ob.preorder()
        nd = bih.nodes
        br = kind != 3
        u = lambda a: np.ascontiguousarray(a).view(np.uint32)
        assert len(nd) == len(kind) and np.array_equal(nd["kind"] & 3, kind), seed
        assert np.array_equal(u(nd["lmax"][br]), u(lmax[br])) and np.array_equal(u(nd["rmin"][br]), u(rmin[br])), seed
        assert np.array_equal((nd["kind"] >> 2)[~br], cnt[~br]), seed
        fl = ob.flatten()
        assert np.array_equal(u(bih.tris["v0"]), u(fl["a"])) and np.array_equal(u(bih.tris["v1"]), u(fl["b"])) and np.array_equal(u(bih.tris["v2"]), u(fl["c"])), seed
        assert np.array_equal(u(bih.bounds), u(np.array(ob.bounds(), np.float32).ravel())), seed


def test_debug_show_prints_haskell_show_text(sqt):
    """--debug prints `head objs` and `mats` with Haskell's derived Show (src/Obj.hs:55-57, 88-94; src/Color.hs:78-83;
    src/V3.hs:5).  `show :: Float`: shortest identifying digits, positional for 0.1 <= x < 10^7, else d.ddde<n>."""
    obj = b"mtllib s.sq\no A\nv 1 2 3\nv 0.05 -0 12345678\nv 100 0.1 9999999\nusemtl M\"x\nf 1 2 3\no B\nv 0 0 0\nusemtl M\"x\nf 1 2 4\n"
    sq = b"newmtl M\"x\nreflective 0.2 1 2 3\nemissive 100 0.608420 0.050408 0\n"
    first, mats = sqt.Mesh.from_text(obj, sq).debug_show()
    assert first == ('Object {verts = [V3 {_x = 1.0, _y = 3.0, _z = 2.0},V3 {_x = 5.0e-2, _y = 1.2345678e7, _z = -0.0},'
                     'V3 {_x = 100.0, _y = 9999999.0, _z = 0.1}], mtl = "M\\"x", faces = [Face {_i1 = 1, _i2 = 2, _i3 = 3}]}')
    assert mats == ('[("M\\"x",Mat {reflective = 0.2, surfColor = V3 {_x = 1.0, _y = 2.0, _z = 3.0}, emissive = 100.0, '
                    'emitColor = V3 {_x = 0.60842, _y = 5.0408e-2, _z = 0.0}})]')
    first, mats = sqt.Mesh.from_obj(os.path.join(DATA, "scene.obj"), DATA).debug_show()
    assert first.startswith("Object {verts = [V3 {_x = 2.0, _y = -2.0, _z = -2.0},V3 {_x = 2.0, _y = 2.0, _z = -2.0},V3 {_x = 2.000001, _y = -1.999999, _z = 2.0}")
    assert first.count("V3 {") == 25 and first.count("Face {") == 32 and 'mtl = "Material.001"' in first
    assert mats.startswith('[("Material.004",Mat {reflective = 0.0, surfColor = V3 {_x = 5.0408e-2, _y = 5.0408e-2, _z = 5.0408e-2}, emissive = 0.0,')
    assert '("Material.002",Mat {reflective = 0.0, surfColor = V3 {_x = 0.0, _y = 0.0, _z = 0.0}, emissive = 100.0, emitColor = V3 {_x = 1.0, _y = 1.0, _z = 1.0}})' in mats
    assert '("Material.005",Mat {reflective = 1.0, surfColor = V3 {_x = 0.8, _y = 0.8, _z = 0.8}' in mats
    tris = np.zeros(1, sqt._native.TRI_DTYPE); m = np.zeros(1, sqt._native.MAT_DTYPE)
    assert sqt.Mesh.from_arrays(tris, m).debug_show() == ("", "")


def test_debug_show_escapes_names_like_showLitChar(sqt):
    """`show :: String` per GHC.Show.showLitChar, on names the reference's `word` token admits (src/Obj.hs:130: anything but
    " \\t\\n\\r\\f\\v"): control characters by their ASCII names, \\DEL, \\SO guarded by \\& before an H, code points above
    127 in decimal (the reference's readFile decodes UTF-8 first) guarded by \\& before a digit, backslash and quote."""
    cases = [("caf\u00e9", 'caf\\233'), ("\u00e91", '\\233\\&1'), ("a\x7fb", 'a\\DELb'), ("x\x0eH", 'x\\SO\\&H'), ("x\x0eI", 'x\\SOI'),
             ("\x01\x07\x08\x1b\x1f", '\\SOH\\a\\b\\ESC\\US'), ("b\\s", 'b\\\\s'), ("\u4e16\u754c9", '\\19990\\30028\\&9'),
             ("\U0001f600", '\\128512'), ("plain.Name_1", 'plain.Name_1')]
    for name, shown in cases:
        raw = name.encode("utf-8")
        obj = b"mtllib s.sq\no A\nv 1 2 3\nv 0 1 0\nv 0 0 1\nusemtl " + raw + b"\nf 1 2 3\n"
        sq = b"newmtl " + raw + b"\nreflective 0 1 1 1\nemissive 0 0 0 0\n"
        first, mats = sqt.Mesh.from_text(obj, sq).debug_show()
        assert f'mtl = "{shown}"' in first, (name, first)
        assert mats.startswith(f'[("{shown}",Mat '), (name, mats)
    # a byte string that is not UTF-8 (the reference's readFile would throw): each byte as the code point of its value
    first, _ = sqt.Mesh.from_text(b"mtllib s.sq\no A\nv 1 2 3\nv 0 1 0\nv 0 0 1\nusemtl \xff\xc3\nf 1 2 3\n",
                                  b"newmtl \xff\xc3\nreflective 0 1 1 1\nemissive 0 0 0 0\n").debug_show()
    assert 'mtl = "\\255\\195"' in first


# ---- independent checks of the host loader and BIH build: nothing below goes through oracle/sq_oracle.c ----
def _numpy_bih_check(bih_nodes, leaf_tris, mesh_tris):
    """Re-derive makeBIH (src/BIH.hs:62-99) in numpy float32 from the INPUT triangles and walk the product's
    pre-order node array beside it: axis (longestAxis, ties -> later axis), split plane (sequential fp32 mean of the
    centroids, strict <), stable partition, lmax / rmin (+-0.001 on the child's vertex extreme), leaf limit 15,
    terminal branches with an empty side, leaf order.  Returns the number of branches checked."""
    f32 = np.float32
    verts_of = lambda t: np.stack([t["v0"], t["v1"], t["v2"]], 1).astype(f32)          # [n, 3 verts, 3 coords]
    pos = [0]          # next pre-order node
    out_first = [0]    # next leaf-order triangle
    checked = [0]

    def leaf(expected):
        nd = bih_nodes[pos[0]]; pos[0] += 1
        assert int(nd["kind"]) & 3 == 3 and int(nd["kind"]) >> 2 == len(expected) and (len(expected) == 0 or int(nd["link"]) == out_first[0])
        got = leaf_tris[out_first[0]: out_first[0] + len(expected)]
        for k in ("v0", "v1", "v2", "mat"):
            assert np.array_equal(got[k], expected[k])
        out_first[0] += len(expected)

    def walk(tris):
        if len(tris) < 15:
            return leaf(tris)
        v = verts_of(tris)
        lo, hi = v.reshape(-1, 3).min(0), v.reshape(-1, 3).max(0)                      # boundingBox of THIS node's triangles
        dims = (hi - lo).astype(f32)
        ax = max(range(3), key=lambda a: (dims[a], a))                                  # maximumBy keeps the last maximum
        cen = (((f32(0) + v[:, 0]) + v[:, 1]) + v[:, 2]) / f32(3)                       # averagePoints (vertices tri)
        plane = (np.cumsum(cen, axis=0, dtype=f32)[-1] / f32(len(tris)))[ax]            # left-to-right fp32 sum, then / n
        under = cen[:, ax] < plane
        left, right = tris[under], tris[~under]
        lmax = f32(0.001) + (verts_of(left)[:, :, ax].max() if len(left) else lo[ax])
        rmin = f32(-0.001) + (verts_of(right)[:, :, ax].min() if len(right) else hi[ax])
        nd = bih_nodes[pos[0]]; me = pos[0]; pos[0] += 1
        assert int(nd["kind"]) == ax, (me, int(nd["kind"]), ax)
        assert nd["lmax"].view(np.uint32) == lmax.view(np.uint32) and nd["rmin"].view(np.uint32) == rmin.view(np.uint32), (me, nd, lmax, rmin)
        checked[0] += 1
        if len(left) == 0 or len(right) == 0:                                           # terminal branch: both children are leaves
            leaf(left)
            assert int(nd["link"]) == pos[0]
            leaf(right)
            return
        walk(left)
        assert int(nd["link"]) == pos[0], "right child index"
        walk(right)

    import sys
    sys.setrecursionlimit(10000)
    walk(mesh_tris)
    assert pos[0] == len(bih_nodes) and out_first[0] == len(leaf_tris) == len(mesh_tris)
    return checked[0]


def test_bih_build_against_a_numpy_rederivation(sqt, product_scene):
    bih, _, mesh = product_scene
    assert _numpy_bih_check(bih.nodes, bih.tris, mesh.tris) == 639                      # scene.obj: 639 branches
    # every triangle is in exactly one leaf: leaf order is a permutation of the input
    key = lambda t: sorted(map(bytes, np.ascontiguousarray(t[["v0", "v1", "v2", "mat"]])))
    assert key(bih.tris) == key(mesh.tris)
    rng = np.random.default_rng(11)
    for n, spread in ((400, 0.3), (60, 1.5), (15, 0.1), (14, 1.0)):
        tris = np.zeros(n, sqt._native.TRI_DTYPE)
        c = rng.uniform(-2, 2, (n, 1, 3))
        v = (c + rng.normal(0, spread, (n, 3, 3))).astype(np.float32)
        tris["v0"], tris["v1"], tris["v2"] = v[:, 0], v[:, 1], v[:, 2]
        m = sqt.Mesh.from_arrays(tris, np.zeros(1, sqt._native.MAT_DTYPE))
        b = sqt.BIH(m)
        _numpy_bih_check(b.nodes, b.tris, m.tris)
    # 40 identical triangles: the centroid mean equals every centroid, nothing is `<` it -> empty left side, terminal branch
    tris = np.zeros(40, sqt._native.TRI_DTYPE)
    tris["v0"], tris["v1"], tris["v2"] = [0, 0, 0], [1, 0, 0], [0, 1, 0.5]
    m = sqt.Mesh.from_arrays(tris, np.zeros(1, sqt._native.MAT_DTYPE))
    b = sqt.BIH(m)
    assert _numpy_bih_check(b.nodes, b.tris, m.tris) == 1 and b.longest_leaf == 40


def _regex_obj_loader(obj_text, sq_text):
    """The .obj / .sq dialect of src/Obj.hs:96-161 read with regular expressions (well-formed files only): objects of
    `v` lines, `usemtl`, optional `s on|off`, `f` lines with 1-based GLOBAL indices; swapYZ; every (object, material)
    pair with equal names, objects outermost (makeScene, src/Obj.hs:73-77)."""
    import re
    num = r"-?\d+(?:\.\d+)?"
    mats = [(m.group(1), [float(x) for x in m.groups()[1:]]) for m in re.finditer(
        rf"newmtl (\S+)\s+reflective ({num})\s+({num})\s+({num})\s+({num})\s+emissive ({num})\s+({num})\s+({num})\s+({num})", sq_text)]
    verts, objects = [], []
    for blk in re.split(r"(?m)^o ", obj_text)[1:]:
        for m in re.finditer(rf"(?m)^v\s+({num})\s+({num})\s+({num})", blk):
            x, y, z = (np.float32(float(g)) for g in m.groups())
            verts.append((x, z, y))                                                   # swapYZ, src/Obj.hs:112-113
        mtl = re.search(r"(?m)^usemtl (\S+)", blk).group(1)
        faces = [tuple(int(g) for g in m.groups()) for m in re.finditer(r"(?m)^f\s+(\d+)\s+(\d+)\s+(\d+)", blk)]
        objects.append((mtl, faces))
    verts = np.array(verts, np.float32)
    out = []
    for mtl, faces in objects:
        for mi, (name, _) in enumerate(mats):
            if name == mtl:
                out += [(verts[a - 1], verts[b - 1], verts[c - 1], mi) for a, b, c in faces]
    return out, mats


def test_loader_against_a_regex_parser(sqt):
    texts = [(open(os.path.join(DATA, "scene.obj"), "rb").read(), open(os.path.join(DATA, "scene.sq"), "rb").read())]
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_scenes
    o, s, _ = gen_scenes.blob_scene(2)
    texts.append((o, s))
    # an object whose material is defined twice is emitted twice; an object without a material is dropped (src/Obj.hs:75)
    texts.append((b"mtllib m.sq\no A\nv 0 0 0\nv 1 0 0\nv 0 1 0\nusemtl Twice\nf 1 2 3\no B\nv 0 0 1\nusemtl Missing\ns on\nf 1 2 4\no C\nv 2 2 2\nusemtl One\ns off\nf 5 4 1\nf 1 2 3\n",
                  b"newmtl Twice\nreflective 0 1 1 1\nemissive 0 0 0 0\n\nnewmtl One\nreflective 1 0.5 0.25 0.125\nemissive 3 1 0 1\n\nnewmtl Twice\nreflective 0.5 0 0 0\nemissive 0 0 0 0\n"))
    for obj, sq in texts:
        want, mats = _regex_obj_loader(obj.decode("latin-1"), sq.decode("latin-1"))
        mesh = sqt.Mesh.from_text(obj, sq)
        got = mesh.tris
        assert len(got) == len(want)
        w0 = np.array([w[0] for w in want], np.float32); w1 = np.array([w[1] for w in want], np.float32); w2 = np.array([w[2] for w in want], np.float32)
        assert np.array_equal(got["v0"].view(np.uint32), w0.view(np.uint32)) and np.array_equal(got["v1"].view(np.uint32), w1.view(np.uint32))
        assert np.array_equal(got["v2"].view(np.uint32), w2.view(np.uint32)) and np.array_equal(got["mat"], [w[3] for w in want])
        gm = mesh.materials
        assert len(gm) == len(mats)
        for g, (_, vals) in zip(gm, mats):
            flat = [g["reflective"], *g["surf"], g["emissive"], *g["emit"]]
            assert np.array_equal(np.array(flat, np.float32).view(np.uint32), np.array(vals, np.float32).view(np.uint32))


def test_bench_without_enough_devices_exits_non_zero():
    """The driver calls `python bench.py --gpus N`.  Without N visible HIP devices (none at all in the CPU container) the
    launcher must fail with a message and print no JSON line: never a silent 1-GPU number labelled N."""
    import subprocess
    import sys
    for n in ("2", "8"):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", n, "--steps", "1", "--warmup", "0"],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
        import torch
        if torch.cuda.device_count() >= int(n):
            continue                                    # a box that really has that many devices runs the benchmark instead
        assert p.returncode == 2 and "device" in p.stderr and p.stdout.strip() == ""
