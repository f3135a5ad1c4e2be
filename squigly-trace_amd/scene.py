"""Host-side data model, mirroring the reference's Obj / Geometry / BIH modules.

    trisFromObj / loadCamera   src/Obj.hs:49-70      -> Mesh.from_obj, load_camera
    makeBIH / flatten          src/BIH.hs:50-52,62-99 -> BIH(mesh)
    height/numLeaves/longestLeaf src/BIH.hs:46-60    -> BIH.height / .num_leaves / .longest_leaf
The arithmetic lives in csrc/sq_host.cpp; these classes only own the C objects.
"""
import ctypes as C

import numpy as np

from . import _native as N


def _records(address, n, dt):
    """A copy of the n records of numpy dtype dt at `address` as an array (n = 0: the address is not looked at)."""
    if n == 0:
        return np.zeros(0, dt)
    buf = (C.c_uint8 * (n * dt.itemsize)).from_address(address)
    return np.frombuffer(buf, dtype=dt).copy()


class Owner:
    """Owns the C object behind the handle _h and hands it back, once, through the library function the subclass names in _free.
    A method and not a function a subclass's module imports: __del__ may run while the interpreter shuts down, when a module's
    globals are already None -- this module's N is looked at for that, and then the handle is only forgotten."""
    _free = None

    def _release(self):
        if getattr(self, "_h", None) and N is not None and N._lib is not None:
            getattr(N._lib, self._free)(self._h)
        self._h = None

    __del__ = _release


class Mesh(Owner):
    """[Triangle] in loader order (Obj.trisFromObj)."""
    _free = "sq_mesh_free"

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def from_obj(cls, obj_path, mtl_dir="./data"):
        h = C.c_void_p()
        N.check(N.lib().sq_mesh_from_obj(str(obj_path).encode(), str(mtl_dir).encode(), C.byref(h)))
        return cls(h)

    @classmethod
    def from_text(cls, obj_text: bytes, sq_text: bytes):
        h = C.c_void_p()
        N.check(N.lib().sq_mesh_from_text(obj_text, len(obj_text), sq_text, len(sq_text), C.byref(h)))
        return cls(h)

    @classmethod
    def from_arrays(cls, tris: np.ndarray, mats: np.ndarray):
        tris = np.ascontiguousarray(tris, dtype=N.TRI_DTYPE)
        mats = np.ascontiguousarray(mats, dtype=N.MAT_DTYPE)
        h = C.c_void_p()
        N.check(N.lib().sq_mesh_from_arrays(tris.ctypes.data, len(tris), mats.ctypes.data, len(mats), C.byref(h)))
        return cls(h)

    def __len__(self):
        return N.lib().sq_mesh_num_tris(self._h)

    def debug_show(self):
        """(`show (head objs)`, `show mats`): the two lines `--debug` prints while loading (src/Obj.hs:55-57)."""
        a, b = C.c_char_p(), C.c_char_p()
        N.lib().sq_mesh_debug_show(self._h, C.byref(a), C.byref(b))
        return (a.value or b"").decode("latin-1"), (b.value or b"").decode("latin-1")

    @property
    def tris(self) -> np.ndarray:
        n = len(self)
        return _records(n and N.lib().sq_mesh_tris(self._h), n, N.TRI_DTYPE)

    @property
    def materials(self) -> np.ndarray:
        n = N.lib().sq_mesh_num_materials(self._h)
        return _records(n and N.lib().sq_mesh_materials(self._h), n, N.MAT_DTYPE)


def moved_mesh(mesh, poses):
    """A Mesh (from_arrays) with the pose of material m applied to every triangle of material m: poses is [n_materials, 3, 4],
    rows [R | t] with world = R local + t, so an identity row leaves a material's triangles where they are, bit for bit.  Computed
    in float64 and rounded to float32 once.  The triangles keep their order and their materials."""
    poses = np.asarray(poses, np.float64)
    mats = mesh.materials
    if poses.ndim != 3 or poses.shape != (len(mats), 3, 4):
        raise ValueError(f"poses must have shape ({len(mats)}, 3, 4): a pose per material, got {poses.shape}")
    tris = np.array(mesh.tris, dtype=N.TRI_DTYPE)
    M = poses[tris["mat"]]                                                     # [n_tris, 3, 4]
    for v in ("v0", "v1", "v2"):
        p = tris[v].astype(np.float64)
        tris[v] = (np.einsum("nij,nj->ni", M[:, :, :3], p) + M[:, :, 3]).astype(np.float32)
    return Mesh.from_arrays(tris, np.array(mats, dtype=N.MAT_DTYPE))


class BIH(Owner):
    """BIH.makeBIH result, flattened to the pre-order arrays of include/squigly_hip.h."""
    _free = "sq_bih_free"

    def __init__(self, mesh: Mesh, device=None):
        """device=None: host build (sq_bih_build); device=k: the same tree built on GPU k (sq_bih_build_device)."""
        h = C.c_void_p()
        if device is None:
            N.check(N.lib().sq_bih_build(mesh._h, C.byref(h)))
        else:
            N.check(N.lib().sq_bih_build_device(mesh._h, int(device), C.byref(h)))
        self._h = h
        self.scene = N.Scene()
        N.lib().sq_bih_scene(self._h, C.byref(self.scene))

    height = property(lambda s: N.lib().sq_bih_height(s._h))
    num_leaves = property(lambda s: N.lib().sq_bih_num_leaves(s._h))
    longest_leaf = property(lambda s: N.lib().sq_bih_longest_leaf(s._h))

    @property
    def nodes(self):
        return _records(self.scene.nodes, self.scene.n_nodes, N.NODE_DTYPE)

    @property
    def tris(self):
        return _records(self.scene.tris, self.scene.n_tris, N.TRI_DTYPE)

    @property
    def materials(self):
        return _records(self.scene.mats, self.scene.n_mats, N.MAT_DTYPE)

    @property
    def bounds(self):
        return np.array(list(self.scene.root.lo) + list(self.scene.root.hi), np.float32)

    def cull_boxes(self):
        """(boxes [n_nodes, 6], (o2max, d2min, d2max)): the culling boxes the device kernels use (sq_cull_boxes)."""
        boxes = np.empty((self.scene.n_nodes, 6), np.float32)
        lim = np.empty(3, np.float32)
        N.check(N.lib().sq_cull_boxes(C.byref(self.scene), boxes.ctypes.data, lim.ctypes.data))
        return boxes, tuple(float(x) for x in lim)


def load_camera(path) -> N.Camera:
    """Obj.loadCamera (src/Obj.hs:60-70)."""
    cam = N.Camera()
    N.check(N.lib().sq_camera_from_file(str(path).encode(), C.byref(cam)))
    return cam


def camera_from_text(text: bytes) -> N.Camera:
    cam = N.Camera()
    N.check(N.lib().sq_camera_from_text(text, len(text), C.byref(cam)))
    return cam


def rot_matrix_rads(a, b, g) -> np.ndarray:
    """Geometry.rotMatrixRads (src/Geometry.hs:90-102), row-major 3x3."""
    out = (C.c_float * 9)()
    N.lib().sq_rot_matrix_rads(a, b, g, out)
    return np.array(list(out), np.float32).reshape(3, 3)
