"""ctypes binding of libsquigly_hip.so (include/squigly_hip.h, include/squigly_host.h).

There is no Python or CPU fallback for the render path: if the shared library is missing this
module raises, and if no HIP device is usable the render entry points return an error.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# SQ_LIB_PATH: development aid, loads an experimental build of the same library (build.py --out=...) for A/B timing
LIB_PATH = os.environ.get("SQ_LIB_PATH") or os.path.join(_HERE, "libsquigly_hip.so")

# numpy mirrors of the C structs
NODE_DTYPE = np.dtype([("kind", "<i4"), ("lmax", "<f4"), ("rmin", "<f4"), ("link", "<i4")])
TRI_DTYPE = np.dtype([("v0", "<f4", 3), ("v1", "<f4", 3), ("v2", "<f4", 3), ("mat", "<i4")])
MAT_DTYPE = np.dtype([("reflective", "<f4"), ("surf", "<f4", 3), ("emissive", "<f4"), ("emit", "<f4", 3)])
assert NODE_DTYPE.itemsize == 16 and TRI_DTYPE.itemsize == 40 and MAT_DTYPE.itemsize == 32


class Bounds(C.Structure):
    _fields_ = [("lo", C.c_float * 3), ("hi", C.c_float * 3)]


class Camera(C.Structure):
    """Geometry.Camera: position + rotation matrix (row-major)."""
    _fields_ = [("pos", C.c_float * 3), ("rot", C.c_float * 9)]


class Scene(C.Structure):
    _fields_ = [("root", Bounds), ("nodes", C.c_void_p), ("n_nodes", C.c_int32), ("tris", C.c_void_p),
                ("n_tris", C.c_int32), ("mats", C.c_void_p), ("n_mats", C.c_int32), ("height", C.c_int32)]


class Shard(C.Structure):
    _fields_ = [("row_block", C.c_int32), ("shard", C.c_int32), ("n_shards", C.c_int32)]


class Light(C.Structure):
    """sq_light: a point light, position and RGB power (the reference's: (0, 3, -1), (2, 2, 2))."""
    _fields_ = [("pos", C.c_float * 3), ("power", C.c_float * 3)]


MAX_LIGHTS = 4096      # sq_scene_set_lights refuses more
MAX_DEPTH = 8          # sq_scene_set_depth refuses more: a path's random words come from one Threefish block


class Plan(C.Structure):
    """sq_plan (include/squigly_hip.h): the launch plan of a scene's last frame."""
    _fields_ = [(n, C.c_int32) for n in ("launched", "variant", "stack_word_bytes", "height", "stack_cap", "trace_form",
                                          "blocks_per_cu", "n_lds", "trace_lds_bytes", "pixel_lds_bytes", "primary_form",
                                          "packed_leaves", "n_emitters", "level1_cull")]


TRACE_FORMS = {0: "per_pixel", 1: "resident", 2: "streaming_six_wave", 3: "streaming_plain"}
PRIMARY_FORMS = {0: "none", 1: "per_lane", 2: "resident", 3: "pooled"}


class SquiglyError(RuntimeError):
    """Raised when a C-ABI call returns non-zero; carries sq_last_error()."""


_lib = None


def load(path):
    """The shared library at `path` (this package's two load through here); ImportError when it was not built."""
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: build it with `python squigly-trace_amd/build.py` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    # PyTorch (the plumbing for device buffers and streams) bundles its own HIP runtime.  It has to be the
    # first HIP runtime loaded into the process: if a library of ours pulls in the system one first, torch's
    # later initialisation reports "No HIP GPUs are available".
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    return C.CDLL(path)


def lib():
    global _lib
    if _lib is not None:
        return _lib
    L = load(LIB_PATH)
    vp, i32, sz = C.c_void_p, C.c_int32, C.c_size_t
    L.sq_last_error.restype = C.c_char_p
    L.sq_device_count.restype = i32
    L.sq_abi_version.restype = i32
    L.sq_build_id.restype = C.c_char_p
    L.sq_render_rgb8.argtypes = [C.POINTER(Scene), C.POINTER(Camera), i32, i32, i32, i32, vp]
    L.sq_render_f32.argtypes = [C.POINTER(Scene), C.POINTER(Camera), i32, i32, i32, i32, vp]
    L.sq_scene_upload.argtypes = [C.POINTER(Scene), i32, C.POINTER(vp)]
    L.sq_scene_free.argtypes = [vp]
    L.sq_scene_free.restype = None
    L.sq_shard_rows.argtypes = [i32, Shard]
    L.sq_shard_rows.restype = i32
    L.sq_shard_global_row.argtypes = [i32, Shard]
    L.sq_shard_global_row.restype = i32
    L.sq_render_rows_device.argtypes = [vp, C.POINTER(Camera), i32, i32, i32, i32, Shard, vp, vp, vp]
    L.sq_render_rows_device_range.argtypes = [vp, C.POINTER(Camera), i32, i32, i32, i32, Shard, i32, i32, vp, vp, vp, vp]
    L.sq_render_rows_device_masked.argtypes = [vp, C.POINTER(Camera), i32, i32, i32, i32, Shard, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    L.sq_adaptive_update_device.argtypes = [vp, C.c_int64, vp, vp, vp, C.c_float, C.c_float, vp, vp, vp]
    L.sq_render_views_device.argtypes = [vp, C.POINTER(Camera), i32, i32, i32, i32, i32, Shard, i32, i32, vp, vp, vp, vp]
    L.sq_intersect_rays_device.argtypes = [vp, vp, vp, C.c_int64, vp, vp, vp, vp]
    L.sq_camera_rays_device.argtypes = [vp, C.POINTER(Camera), i32, i32, Shard, vp, vp, vp]
    L.sq_raytrace_rays_device.argtypes = [vp, vp, vp, vp, C.c_int64, i32, i32, vp, vp, vp, vp]
    L.sq_raycast_rays_device.argtypes = [vp, vp, vp, C.c_int64, vp, vp]
    L.sq_scene_set_lights.argtypes = [vp, vp, i32, vp]
    L.sq_scene_get_lights.argtypes = [vp, vp, i32]
    L.sq_scene_get_lights.restype = i32
    L.sq_scene_set_depth.argtypes = [vp, i32]
    L.sq_scene_get_depth.argtypes = [vp]
    L.sq_scene_get_depth.restype = i32
    L.sq_scene_set_sky.argtypes = [vp, vp]
    L.sq_scene_get_sky.argtypes = [vp, vp]
    L.sq_kernel_timing.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_char_p)]
    L.sq_kernel_timing_reset.argtypes = [vp]
    L.sq_kernel_timing_reset.restype = None
    L.sq_set_option.argtypes = [vp, C.c_char_p, C.c_int64]
    L.sq_scene_rng_table.argtypes = [vp, C.c_int64, C.c_int64, vp]
    L.sq_scene_rng_table.restype = C.c_int64
    L.sq_rng_table_cover.argtypes = [i32, i32, i32, C.c_int64]
    L.sq_rng_table_cover.restype = C.c_int64
    L.sq_get_stats.argtypes = [vp, C.POINTER(C.c_uint64), i32, i32]
    L.sq_last_plan.argtypes = [vp, C.POINTER(Plan)]
    L.sq_debug_eval.argtypes = [i32, i32, vp, vp, C.c_int64, vp]
    # host side
    L.sq_mesh_from_obj.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(vp)]
    L.sq_mesh_from_text.argtypes = [C.c_char_p, sz, C.c_char_p, sz, C.POINTER(vp)]
    L.sq_mesh_from_arrays.argtypes = [vp, i32, vp, i32, C.POINTER(vp)]
    L.sq_mesh_num_tris.argtypes = [vp]
    L.sq_mesh_num_materials.argtypes = [vp]
    L.sq_mesh_tris.argtypes = [vp]
    L.sq_mesh_tris.restype = vp
    L.sq_mesh_materials.argtypes = [vp]
    L.sq_mesh_materials.restype = vp
    L.sq_mesh_free.argtypes = [vp]
    L.sq_mesh_free.restype = None
    L.sq_camera_from_file.argtypes = [C.c_char_p, C.POINTER(Camera)]
    L.sq_camera_from_text.argtypes = [C.c_char_p, sz, C.POINTER(Camera)]
    L.sq_rot_matrix_rads.argtypes = [C.c_float, C.c_float, C.c_float, C.POINTER(C.c_float)]
    L.sq_rot_matrix_rads.restype = None
    L.sq_mesh_debug_show.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p)]
    L.sq_mesh_debug_show.restype = None
    L.sq_release_cached_memory.argtypes = []
    L.sq_release_cached_memory.restype = None
    L.sq_bih_build.argtypes = [vp, C.POINTER(vp)]
    L.sq_bih_build_device.argtypes = [vp, C.c_int32, C.POINTER(vp)]
    L.sq_cull_boxes.argtypes = [C.POINTER(Scene), vp, vp]
    L.sq_half_outward.argtypes = [C.c_float, i32]
    L.sq_half_outward.restype = C.c_uint32
    L.sq_scene_pack.argtypes = [C.POINTER(Scene), C.POINTER(vp)]
    L.sq_packed_array.argtypes = [vp, C.c_char_p, C.POINTER(vp), C.POINTER(sz)]
    L.sq_packed_scalar.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int64)]
    L.sq_packed_free.argtypes = [vp]
    L.sq_packed_free.restype = None
    if hasattr(L, "sq_plan_call"):       # (a library from before the planner's window, timed against this one through SQ_LIB_PATH, has none)
        L.sq_plan_call.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_int64), i32, C.c_int64, C.POINTER(Plan),
                                   C.POINTER(C.c_char_p), C.POINTER(C.c_int64), i32]
    L.sq_bih_scene.argtypes = [vp, C.POINTER(Scene)]
    L.sq_bih_scene.restype = None
    for f in ("height", "num_leaves", "longest_leaf"):
        getattr(L, "sq_bih_" + f).argtypes = [vp]
        getattr(L, "sq_bih_" + f).restype = i32
    L.sq_bih_free.argtypes = [vp]
    L.sq_bih_free.restype = None
    _lib = L
    return L


# The reference's hard-coded light (src/Lib.hs:141-151) as a row of DeviceScene.lights: position, then RGB power.
REFERENCE_LIGHT = ((0.0, 3.0, -1.0), (2.0, 2.0, 2.0))


def lights_array(lights):
    """The float32 [n, 6] array (pos, power) of DeviceScene.set_lights' argument: an array-like [n, 6], or a sequence of
    (pos, power) pairs, power a scalar or three numbers.  SquiglyError for any other shape, no light or more than MAX_LIGHTS."""
    try:
        seq = list(lights)
    except TypeError:
        raise SquiglyError(f"lights must be an [n, 6] array or a sequence of (pos, power) pairs, got {type(lights).__name__}")
    if len(seq) == 0:
        raise SquiglyError("lights must hold at least one light (None restores the reference's light)")
    if len(seq) > MAX_LIGHTS:
        raise SquiglyError(f"{len(seq)} lights are too many (at most {MAX_LIGHTS})")
    rows = []
    for i, item in enumerate(seq):
        try:
            if len(item) == 2:                        # (pos, power)
                pos = np.asarray(item[0], np.float32).reshape(-1)
                power = np.asarray(item[1], np.float32).reshape(-1)
                if power.size == 1:
                    power = np.repeat(power, 3)
                row = np.concatenate([pos, power]) if pos.size == 3 and power.size == 3 else None
            else:
                row = np.asarray(item, np.float32).reshape(-1)
        except (TypeError, ValueError):
            row = None
        if row is None or row.shape != (6,):
            raise SquiglyError(f"light {i}: expected (pos, power) with three coordinates and a power of one or three numbers, "
                               f"or six numbers, got {item!r}")
        rows.append(row)
    return np.ascontiguousarray(np.stack(rows), np.float32)


def depth_value(depth):
    """The int of a path depth (DeviceScene.set_depth, depth= of the render functions); SquiglyError for anything that is not an
    integer in 1 .. MAX_DEPTH (a bool and a float, integral or not, are not integers here)."""
    from . import _plumbing as P              # (it imports this module)
    if not P.is_integer(depth):
        raise SquiglyError(f"depth must be an integer in 1..{MAX_DEPTH}, got {depth!r}")
    if not 1 <= int(depth) <= MAX_DEPTH:
        raise SquiglyError(f"depth must be in 1..{MAX_DEPTH} (got {int(depth)})")
    return int(depth)


def sky_value(up, down=None):
    """The float32 array [2, 3] (up, down) of DeviceScene.set_sky's arguments and of sky= of the render functions: up and down are
    three numbers each, down = None is up once more (a constant sky).  The values are not checked (NaN, infinite and negative
    components are inputs like any other); SquiglyError for anything that is not three numbers."""
    rows = []
    for name, v in (("up", up), ("down", up if down is None else down)):
        try:
            row = np.asarray(v, np.float32).reshape(-1)
        except (TypeError, ValueError):
            row = None
        if row is None or row.shape != (3,) or isinstance(v, (str, bytes)):
            raise SquiglyError(f"sky {name}: expected three numbers (R, G, B), got {v!r}")
        rows.append(row)
    return np.ascontiguousarray(np.stack(rows), np.float32)


def sky_pair(sky):
    """sky= of the render functions and of a checkpoint -- None, three numbers (a constant sky) or (up, down) -- as None or the
    float32 array [2, 3]."""
    if sky is None:
        return None
    try:
        n = len(sky)
    except TypeError:
        raise SquiglyError(f"sky must be None, three numbers or (up, down), got {sky!r}")
    if n == 2:
        return sky_value(sky[0], sky[1])
    return sky_value(sky)


OPS = {"sqrt": 0, "div": 1, "sin": 2, "cos": 3, "acos": 4, "atan": 5, "unit_float": 6, "tfgen3": 7, "tonemap": 8, "rcp_sweep": 9, "cull_slab": 10}


def debug_eval(op, a, b=None, device=0):
    """sq_debug_eval: one primitive of the numeric spec evaluated on the GPU (diagnostics)."""
    code = OPS[op]
    if op == "tfgen3":
        a = np.ascontiguousarray(a, np.int64); n = a.size; out = np.empty((n, 3), np.uint32)
    elif op == "tonemap":
        a = np.ascontiguousarray(a, np.float32).reshape(-1, 3); n = len(a); out = np.empty((n, 3), np.uint8)
    elif op == "unit_float":
        a = np.ascontiguousarray(a, np.uint32); n = a.size; out = np.empty(n, np.float32)
    elif op == "cull_slab":
        a = np.ascontiguousarray(a, np.uint32).reshape(-1, 9); n = len(a); out = np.empty(n, np.uint32)
    elif op == "rcp_sweep":
        a = np.ascontiguousarray(a, np.uint32); n = a.size; out = np.empty(n, np.uint32)
    else:
        a = np.ascontiguousarray(a, np.float32); n = a.size; out = np.empty(n, np.float32)
    if b is not None:
        b = np.ascontiguousarray(b, np.float32)
    check(lib().sq_debug_eval(device, code, a.ctypes.data, b.ctypes.data if b is not None else None, n, out.ctypes.data))
    return out


def build_id():
    """sq_build_id(): hash of the sources and flags the loaded library was built from (build.py: source_id)."""
    return lib().sq_build_id().decode()


def checked(rc, last_error, count=False):
    """rc, the return value of a C-ABI call, or SquiglyError with what the library's `last_error` function says: non-zero is an
    error; of a call that returns a count (count=True), a negative value is."""
    if (rc < 0) if count else (rc != 0):
        raise SquiglyError(last_error().decode(errors="replace"))
    return rc


def check(rc):
    checked(rc, lib().sq_last_error)


def count(n):
    """The count a getter of libsquigly_hip.so returned; SquiglyError for a negative one."""
    return checked(n, lib().sq_last_error, count=True)


class Binding:
    """One of the package's other shared libraries, bound once: where it is, how it is loaded, and the two functions
    every library has, sq_<name>_last_error and sq_<name>_build_id.  A module takes its LIB_PATH, lib, check and build_id from here:

        LIB_PATH, lib, check, build_id = N.Binding("libsquigly_lens.so", "sq_lens_", _declare, env="SQ_LENS_LIB_PATH", client=True)

    file: the library's name beside this file; env: an environment variable that names another build of the same library (a
    development aid: build.py's compile_lib(..., out=...)); declare(L): sets the argtypes and restypes of the library's own functions;
    client: the library is linked against libsquigly_hip.so, which is then loaded from this package first."""

    def __init__(self, file, prefix, declare, env=None, client=False):
        self.path = (os.environ.get(env) if env else None) or os.path.join(_HERE, file)
        self.prefix, self.declare, self.client, self._lib = prefix, declare, client, None

    def __iter__(self):
        return iter((self.path, self.lib, self.check, self.build_id))

    def load(self, path):
        """The build of the library at `path`, with its prototypes declared (a variant beside the product's)."""
        if self.client:
            lib()
        L = load(path)
        getattr(L, self.prefix + "last_error").restype = C.c_char_p
        getattr(L, self.prefix + "build_id").restype = C.c_char_p
        self.declare(L)
        return L

    def lib(self):
        if self._lib is None:
            self._lib = self.load(self.path)
        return self._lib

    def check(self, rc):
        checked(rc, getattr(self.lib(), self.prefix + "last_error"))

    def entry(self, name):
        """The library's function `name` as a call that raises SquiglyError with the library's message when it returns non-zero.
        Made once per entry point, at import: the library is loaded by the first call, not here."""
        err = self.prefix + "last_error"

        def call(*args):
            L = self.lib()
            checked(getattr(L, name)(*args), getattr(L, err))
        return call

    def build_id(self):
        """sq_<name>_build_id(): hash of the sources and flags the loaded library was built from (build.py: lib_source_id)."""
        return getattr(self.lib(), self.prefix + "build_id")().decode()


EXPORTED_SYMBOLS = [
    # include/squigly_hip.h
    "sq_render_rgb8", "sq_render_f32", "sq_scene_upload", "sq_scene_free", "sq_shard_rows",
    "sq_shard_global_row", "sq_render_rows_device", "sq_render_rows_device_range", "sq_render_rows_device_masked", "sq_adaptive_update_device", "sq_render_views_device", "sq_intersect_rays_device", "sq_camera_rays_device", "sq_raytrace_rays_device", "sq_raycast_rays_device", "sq_scene_set_lights", "sq_scene_get_lights", "sq_scene_set_depth", "sq_scene_get_depth", "sq_scene_set_sky", "sq_scene_get_sky", "sq_kernel_timing", "sq_kernel_timing_reset",
    "sq_set_option", "sq_scene_rng_table", "sq_get_stats", "sq_last_plan", "sq_debug_eval", "sq_device_count", "sq_abi_version", "sq_build_id", "sq_last_error",
    # include/squigly_host.h
    "sq_mesh_from_obj", "sq_mesh_from_text", "sq_mesh_from_arrays", "sq_mesh_num_tris",
    "sq_mesh_num_materials", "sq_mesh_tris", "sq_mesh_materials", "sq_mesh_free", "sq_camera_from_file",
    "sq_camera_from_text", "sq_rot_matrix_rads", "sq_release_cached_memory", "sq_mesh_debug_show", "sq_bih_build", "sq_bih_build_device", "sq_cull_boxes", "sq_half_outward", "sq_scene_pack", "sq_packed_array", "sq_packed_scalar", "sq_packed_free", "sq_plan_call", "sq_rng_table_cover", "sq_bih_scene", "sq_bih_height",
    "sq_bih_num_leaves", "sq_bih_longest_leaf", "sq_bih_free",
]
