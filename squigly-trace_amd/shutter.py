"""ctypes binding of libsquigly_shutter.so (include/squigly_shutter.h) and the helpers around it: motion blur.

A shutter frame is a lens frame (lens.py, mlens.py) whose camera moves while the shutter is open: the R sub-rays of a pixel are R
consecutive instants of the exposure, each under the pose of its own instant.  PyTorch is the plumbing (device memory, streams);
every ray and every pose on the device comes from the HIP kernels of csrc/sq_shutter.hip and every sample from libsquigly_hip.so's
radiance query.  There is no fallback: a missing library raises.
"""
import ctypes as C
import math
import re

from . import _native as N
from . import lens as LN

# include/squigly_shutter.h
EXPORTED_SYMBOLS = ["sq_shutter_last_error", "sq_shutter_build_id", "sq_shutter_pose", "sq_shutter_rays_device", "sq_shutter_render_device"]

_NUMBER = re.compile(rb"-?[0-9]+(?:\.[0-9]+)?")


def _camera_file_numbers(text):
    """The six numbers of a camera file -- position, then rotMatrixRads' angles -- as the library reads them: the text must be one
    sq_camera_from_text takes (SquiglyError with its message otherwise), and each number is strtof's correctly rounded float."""
    if isinstance(text, str):
        text = text.encode()
    N.check(N.lib().sq_camera_from_text(text, len(text), C.byref(N.Camera())))
    strtof = C.CDLL(None).strtof
    strtof.restype, strtof.argtypes = C.c_float, [C.c_char_p, C.c_void_p]
    vals = [float(strtof(tok, None)) for tok in _NUMBER.findall(text)[:6]]
    return vals[:3], vals[3:]


def _pose(name, v):
    """(pos, angles) of `open` / `close`: a pair of three numbers each, or the text of a camera file."""
    if isinstance(v, (bytes, str)):
        return _camera_file_numbers(v)
    try:
        pos, ang = v
        pos, ang = [float(x) for x in pos], [float(x) for x in ang]
    except (TypeError, ValueError):
        raise N.SquiglyError(f"{name} must be (position, angles), three numbers each, or the text of a camera file; got {v!r}")
    if len(pos) != 3 or len(ang) != 3:
        raise N.SquiglyError(f"{name} must be (position, angles), three numbers each, or the text of a camera file; got {v!r}")
    return pos, ang


class Motion(C.Structure):
    """sq_motion: the camera as the shutter opens and as it closes -- each a position and rotMatrixRads' three angles, given as a
    pair (pos, angles) or as the text of a camera file -- and time_jitter (0..1: how much of its own 1/R of the exposure a sub-ray's
    instant is drawn from; 0 = its start, 1 = all of it).  Positions and angles are not checked, as sky and light values are not;
    SquiglyError for a time_jitter the library would refuse."""
    _fields_ = [("pos0", C.c_float * 3), ("ang0", C.c_float * 3), ("pos1", C.c_float * 3), ("ang1", C.c_float * 3),
                ("time_jitter", C.c_float)]

    def __init__(self, open, close, time_jitter=1.0):
        if isinstance(time_jitter, bool) or not isinstance(time_jitter, (int, float)):
            raise N.SquiglyError(f"time_jitter must be a number, got {time_jitter!r}")
        t = float(time_jitter)
        if not 0.0 <= t <= 1.0:
            raise N.SquiglyError(f"time_jitter must be a number in [0, 1] (got {t!r})")
        (p0, a0), (p1, a1) = _pose("open", open), _pose("close", close)
        f3 = C.c_float * 3
        super().__init__(f3(*p0), f3(*a0), f3(*p1), f3(*a1), t)

    def pose(self, t):
        """sq_shutter_pose: the Camera at the instant t of the exposure (0 = open, 1 = close), from the host code the kernels share."""
        cam = N.Camera()
        check(lib().sq_shutter_pose(C.byref(self), float(t), C.byref(cam)))
        return cam

    def key(self):
        """The motion as bytes: two motions are the same when their bits are (a NaN component equals itself)."""
        return bytes(self)

    def __repr__(self):
        return (f"Motion(open=({list(self.pos0)!r}, {list(self.ang0)!r}), close=({list(self.pos1)!r}, {list(self.ang1)!r}), "
                f"time_jitter={self.time_jitter!r})")


def _declare(L):
    vp, i32, i64, sz = C.c_void_p, C.c_int32, C.c_int64, C.c_size_t
    L.sq_shutter_pose.argtypes = [C.POINTER(Motion), C.c_float, C.POINTER(N.Camera)]
    frame = [C.POINTER(Motion), C.POINTER(LN.Lens)] + 6 * [i32] + [N.Shard]
    L.sq_shutter_rays_device.argtypes = [i32] + frame + [vp, i64, vp, vp, vp, vp]
    L.sq_shutter_render_device.argtypes = [vp] + frame + [vp, i64, vp, sz, vp, vp, vp, vp, vp, vp]


# SQ_SHUTTER_LIB_PATH: development aid, loads an experimental build of the same library (build.py: compile_lib(LIBS["shutter"], out=...))
_B = N.Binding("libsquigly_shutter.so", "sq_shutter_", _declare, env="SQ_SHUTTER_LIB_PATH", client=True)
LIB_PATH, lib, check, build_id = _B
_RAYS, _RENDER = _B.entry("sq_shutter_rays_device"), _B.entry("sq_shutter_render_device")


def motion_arg(motion):
    """motion as it is; SquiglyError, before any device work, unless it is a Motion the library would take."""
    if not isinstance(motion, Motion):
        raise N.SquiglyError(f"motion must be a Motion, got {type(motion).__name__}")
    t = motion.time_jitter
    if not (0.0 <= t <= 1.0 and math.isfinite(t)):
        raise N.SquiglyError(f"time_jitter must be a number in [0, 1] (got {t!r})")
    return motion


# The three calls are lens.py's drivers under a motion in the camera's place; a dense call leaves the entry points' list empty.
def shutter_rays(ds, motion, lens, samples, subrays, w, h, shard=(None, 0, 1), r_range=None, stream=None):
    """DeviceScene.shutter_rays: lens.lens_rays under a moving camera (sq_shutter_rays_device, dense): (origins, directions, seeds),
    float32 CUDA tensors [nb, rows, h, 3] and int64 [nb, rows, h], nb = r_end - r_begin."""
    return LN.frame_rays(_RAYS, motion_arg(motion), ds, lens, samples, subrays, w, h, shard, r_range, stream, list_slot=True)


def render_shutter(ds, motion, lens, samples, subrays, w, h, shard=(None, 0, 1), r_range=None, sums=None, want_sum2=False, want_avg=True,
                   want_rgb=True, work_mb=None, stream=None):
    """DeviceScene.render_shutter: lens.render_lens under a moving camera (sq_shutter_render_device, dense); returns
    LensFrame(sum, sum2, avg, rgb), enqueued on `stream`.  Every argument but `motion` is render_lens'."""
    return LN.frame_dense(_RENDER, "render_shutter", motion_arg(motion), ds, lens, samples, subrays, w, h, shard, r_range, sums, want_sum2,
                          want_avg, want_rgb, work_mb, stream, list_slot=True)


def render_shutter_masked(ds, motion, lens, samples, subrays, w, h, r_begin, r_end, sums, index, n_live, sums2=None, counts=None,
                          shard=(None, 0, 1), work_mb=None, out_avg=None, out_rgb=None, stream=None):
    """DeviceScene.render_shutter_masked: mlens.render_lens_masked under a moving camera (sq_shutter_render_device with a list);
    returns (out_avg, out_rgb) as given.  Every argument but `motion` is render_lens_masked's; the list is live_pixels'."""
    return LN.frame_listed(_RENDER, "render_shutter_masked", motion_arg(motion), ds, lens, samples, subrays, w, h, r_begin, r_end, sums,
                           index, n_live, sums2, counts, shard, work_mb, out_avg, out_rgb, stream)

