"""Scenes and cameras that more than one test module renders, and the packed form of a scene.

Belongs here: a camera text, a material set, a generated or padded scene, or a factory that opens one on the device, as soon as a
second file needs it.  Generators draw from default_rng(seed) in a fixed order: goldens, recorded seeds and the counts tests assert
depend on it, so a generator here is never reordered, only added to at the end.  Importing this module loads no native library."""
import ctypes as C
import os

import numpy as np

import tree_padding as TP

DATA = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data")

# ---- cameras -----------------------------------------------------------------------------------------------------------------
ROTATED = b"0 7 0.75\n1.4 0.15 0.2\n"
SOUP_CAMERA = b"-6 0.1 0.2\n0 0 0\n"               # sees the emitter soups with empty space around them


def camera(sqt, which):
    """data/camera ("camera") or ROTATED as a product camera."""
    return sqt.camera_from_text(open(os.path.join(DATA, "camera"), "rb").read() if which == "camera" else ROTATED)


# ---- materials ---------------------------------------------------------------------------------------------------------------
# data/scene.sq with light everywhere: five of the six materials emit a little, each with a colour of its own, and every surface
# colour but the lamp's is non-zero and distinct, so a path's radiance tells which surfaces it met.  The 1.0 and 0.2 mirrors stay.
BRIGHT_SQ = b"""newmtl Material.004
reflective 0 0.350408 0.250408 0.450408
emissive 0.5 0.3 0.6 0.9

newmtl Material.001
reflective 0.2 0.043584 0.258515 0.321582
emissive 0.25 0.9 0.5 0.2

newmtl Material.003
reflective 0.2 0.608420 0.508420 0.408420
emissive 0.125 0.2 0.9 0.4

newmtl Material.002
reflective 0 0 0 0
emissive 100 1 1 1

newmtl Material
reflective 0.2 0.515584 0.024571 0.104109
emissive 0 0 0 0

newmtl Material.005
reflective 1 0.80000 0.70000 0.60000
emissive 0.75 0.6 0.2 0.7
"""


def oracle_tris_of(O, v, mats, mat):
    """The oracle's triangle records of vertices [n, 3, 3], a material table and each triangle's material index."""
    ot = np.zeros(len(v), O.TRI_DTYPE)
    ot["a"], ot["b"], ot["c"] = v[:, 0], v[:, 1], v[:, 2]
    for f in ("reflective", "surf", "emissive", "emit"):
        ot[f] = mats[f][mat]
    return ot


def oracle_tris(O, tris, mats):
    """The oracle's triangle records of a product mesh's arrays."""
    return oracle_tris_of(O, np.stack([tris["v0"], tris["v1"], tris["v2"]], 1), mats, tris["mat"])


# ---- generated scenes --------------------------------------------------------------------------------------------------------
def emitter_soup(sqt, seed, n_emit):
    """A soup of 400 triangles with diffuse, half-mirror and full-mirror materials and n_emit emitting triangles:
    (tris, mats, v, mat).  tests/test_pack.py packs the same soups on the CPU."""
    rng = np.random.default_rng(seed)
    n = 400
    c = rng.uniform(-1.5, 1.5, (n, 1, 3))
    v = (c + rng.normal(0, 0.35, (n, 3, 3))).astype(np.float32)
    mats = np.zeros(4, sqt._native.MAT_DTYPE)
    mats["reflective"] = [0.0, 0.5, 1.0, 0.0]
    mats["surf"] = [[0.7, 0.6, 0.5], [0.4, 0.8, 0.6], [0.9, 0.9, 0.9], [0.0, 0.0, 0.0]]
    mats["emissive"] = [0, 0, 0, 25]
    mats["emit"] = [[0, 0, 0], [0, 0, 0], [0, 0, 0], [1.0, 0.8, 0.6]]
    mat = rng.integers(0, 3, n)
    mat[rng.choice(n, n_emit, replace=False)] = 3
    tris = np.zeros(n, sqt._native.TRI_DTYPE)
    tris["v0"], tris["v1"], tris["v2"], tris["mat"] = v[:, 0], v[:, 1], v[:, 2], mat
    return tris, mats, v, mat


def emitter_soup_scene(sqt, O, seed, n_emit):
    """emitter_soup as (product BIH, oracle BIH, product camera, oracle camera); the camera sees empty space around it."""
    tris, mats, v, mat = emitter_soup(sqt, seed, n_emit)
    ob = O.BIH(oracle_tris_of(O, v, mats, mat))
    return sqt.BIH(sqt.Mesh.from_arrays(tris, mats)), ob, sqt.camera_from_text(SOUP_CAMERA), O.camera_from_text(SOUP_CAMERA)


def overflow_room_obj():
    """A closed cube room of absorbing walls (material Black) with a lamp quad (material Sun) inside, as .obj text."""
    r = 3
    corners = [(x, y, z) for x in (-r, r) for y in (-r, r) for z in (-r, r)]
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    out = ["mtllib scene.sq", "o Room"] + ["v %d %d %d" % c for c in corners] + ["usemtl Black", "s off"]
    for a, b, c, d in quads:
        out += ["f %d %d %d" % (a + 1, b + 1, c + 1), "f %d %d %d" % (a + 1, c + 1, d + 1)]
    out += ["o Lamp", "v -2 2.5 -2", "v 2 2.5 -2", "v 2 2.5 2", "v -2 2.5 2", "usemtl Sun", "s off", "f 9 10 11", "f 9 11 12"]
    return ("\n".join(out) + "\n").encode()


def overflow_room(sqt, O):
    """The room of test_gpu_parity.test_overflowing_emission_defeats_the_absorbing_shortcut with an emission product that
    overflows (1e30 * 1e30): the reference's 0 * inf = NaN reaches the fold."""
    obj = overflow_room_obj()
    big = b"1" + b"0" * 30
    sq = (b"newmtl Black\nreflective 0 0 0 0\nemissive 0 0 0 0\n\n"
          b"newmtl Sun\nreflective 0 0 0 0\nemissive " + big + b" " + big + b" " + big + b" " + big + b"\n")
    cam_txt = b"0 0 0\n0 0 0\n"
    return (sqt.BIH(sqt.Mesh.from_text(obj, sq)), O.BIH(O.tris_from_text(obj, sq)), sqt.camera_from_text(cam_txt),
            O.camera_from_text(cam_txt))


# ---- data/scene.obj at the kernels' limits (tests/test_gpu_limits.py; tests/test_tree_padding.py checks the premises) -------------
LIMITS_W, LIMITS_H = 32, 24                         # the frame of the limit tests


def near_of(O, cam_o):
    """(axis, side) that every primary ray of the LIMITS_W x LIMITS_H frame visits first (tree_padding.full_stack orients by it)."""
    return TP.near_side([O.make_ray(LIMITS_W, LIMITS_H, y, x, cam_o)[1] for y in range(LIMITS_W) for x in range(LIMITS_H)])


def tall_u32(bih0, height, axis, side):
    """tree_padding.full_stack of scene.obj at `height` under one more wrapper whose other child is a balanced empty subtree
    that takes the branch count to exactly 0x9000: the deep branches of the scene and of the frame-filling chain come after
    the empty subtree's in the device's breadth-first numbering, above 0x8000."""
    nb0 = int(((bih0.nodes["kind"] & 3) != 3).sum())
    inner = TP.full_stack_wrappers(bih0, height - 1, axis, side)
    n_empty = 0x9000 - nb0 - len(inner) - 12 - 1
    return TP.PaddedScene(bih0, {0: [(axis, side, ("balanced", n_empty))] + inner})


def big_leaf(sqt, O, base_bih, cam_o, count):
    """scene.obj plus count - 1 copies of the triangle the centre ray hits, forming one leaf of `count` members: each copy
    has a material of its own, so the winner of the exact ties (minimumBy keeps the first) shows in the image, and the last
    copy sits 1e-6 nearer the camera, so it wins wherever it is tested -- only if the whole leaf is."""
    o, d = O.make_ray(LIMITS_W, LIMITS_H, LIMITS_W // 2, LIMITS_H // 2, cam_o)
    hit = O.BIH(O.tris_from_obj(os.path.join(DATA, "scene.obj"), DATA)).intersect(o, d).tri
    mesh = sqt.Mesh.from_obj(os.path.join(DATA, "scene.obj"), DATA)
    tris, mats = mesh.tris, mesh.materials
    extra = np.zeros(count - 1, mats.dtype)
    extra["surf"] = np.stack([np.linspace(0.2, 0.9, count - 1), np.linspace(0.9, 0.2, count - 1), np.full(count - 1, 0.5)], 1)
    copies = np.repeat(base_bih.tris[hit:hit + 1], count - 1)
    copies["mat"] = len(mats) + np.arange(count - 1)
    for k in ("v0", "v1", "v2"):
        copies[k][-1] = (copies[k][-1] - np.float32(1e-6) * d).astype(np.float32)
    return np.concatenate([tris, copies]), np.concatenate([mats, extra])


# ---- a restatement's case on the device --------------------------------------------------------------------------------------
class Scene:
    pass


def open_case(sqt, case, case_paths):
    """A depth_restatement.case with its paths (case_paths: the walk of the restatement that will judge it) and a DeviceScene of its
    own; `want` caches expected values.  The caller closes s.ds."""
    s = Scene()
    s.c = case
    s.paths = case_paths(s.c)
    s.ds = sqt.DeviceScene(s.c.bih, 0)
    s.want = {}
    return s


# ---- the packed scene (sq_scene_pack, include/squigly_host.h) ----------------------------------------------------------------------
ARRAYS = ["branches", "leaves", "tris", "tri_mat", "surfs", "mats", "verts4", "trix", "rbranch", "emitters", "cull_child",
          "cull_child16", "branches_m"]
SCALARS = ["n_branches", "n_leaves", "height", "root_ref", "rroot", "packed_leaves", "nonneg_materials", "finite_geometry",
           "n_emitters", "n_verts", "cull_o2max", "cull_d2min", "cull_d2max", "small_index"]


def pack(sqt, holder):
    """sq_scene_pack of holder.scene (the holder keeps the arrays alive): ({array name: bytes}, {scalar name: int})."""
    L, h = sqt.lib(), C.c_void_p()
    sqt._native.check(L.sq_scene_pack(C.byref(holder.scene), C.byref(h)))
    try:
        arrays, scalars = {}, {}
        for name in ARRAYS:
            data, n = C.c_void_p(), C.c_size_t()
            assert L.sq_packed_array(h, name.encode(), C.byref(data), C.byref(n)) == 0, name
            arrays[name] = C.string_at(data, n.value) if n.value else b""
        for name in SCALARS:
            v = C.c_int64()
            assert L.sq_packed_scalar(h, name.encode(), C.byref(v)) == 0, name
            scalars[name] = v.value
        assert L.sq_packed_array(h, b"rtail", C.byref(data), C.byref(n)) != 0          # unknown names are refused
        assert L.sq_packed_scalar(h, b"incremental_ok", C.byref(v)) != 0
    finally:
        L.sq_packed_free(h)
    return arrays, scalars


LEVEL1_ARRAYS = ["level1", "level1_cover", "level1_mirror"]        # younger than the recorded digests of ARRAYS and SCALARS: a golden of their own
LEVEL1_SCALARS = ["level1_on", "level1_zero", "shortcut_depth"]


def pack_level1(sqt, holder):
    """pack's sibling for the level-1 records: ({name: bytes} of LEVEL1_ARRAYS, {name: int} of LEVEL1_SCALARS)."""
    L, h = sqt.lib(), C.c_void_p()
    sqt._native.check(L.sq_scene_pack(C.byref(holder.scene), C.byref(h)))
    try:
        arrays, scalars = {}, {}
        for name in LEVEL1_ARRAYS:
            data, n = C.c_void_p(), C.c_size_t()
            assert L.sq_packed_array(h, name.encode(), C.byref(data), C.byref(n)) == 0, name
            arrays[name] = C.string_at(data, n.value) if n.value else b""
        for name in LEVEL1_SCALARS:
            v = C.c_int64()
            assert L.sq_packed_scalar(h, name.encode(), C.byref(v)) == 0, name
            scalars[name] = v.value
    finally:
        L.sq_packed_free(h)
    return arrays, scalars
