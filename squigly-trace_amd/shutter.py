"""ctypes binding of libsquigly_shutter.so (include/squigly_shutter.h) and the helpers around it: motion blur.

A shutter frame is a lens frame (lens.py, mlens.py) whose camera moves while the shutter is open: the R sub-rays of a pixel are R
consecutive instants of the exposure, each under the pose of its own instant.  PyTorch is the plumbing (device memory, streams);
every ray and every pose on the device comes from the HIP kernels of csrc/sq_shutter.hip and every sample from libsquigly_hip.so's
radiance query.  There is no fallback: a missing library raises.
"""
import ctypes as C
import math
import os
import re

from . import _native as N
from . import _plumbing as P
from . import lens as LN

_HERE = os.path.dirname(os.path.abspath(__file__))
# SQ_SHUTTER_LIB_PATH: development aid, loads an experimental build of the same library (build.py: build_shutter(out=...))
LIB_PATH = os.environ.get("SQ_SHUTTER_LIB_PATH") or os.path.join(_HERE, "libsquigly_shutter.so")

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


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    N.lib()                                   # the library it is a client of, loaded from this package first
    L = N.load(LIB_PATH)
    vp, i32, i64, sz = C.c_void_p, C.c_int32, C.c_int64, C.c_size_t
    L.sq_shutter_last_error.restype = C.c_char_p
    L.sq_shutter_build_id.restype = C.c_char_p
    L.sq_shutter_pose.argtypes = [C.POINTER(Motion), C.c_float, C.POINTER(N.Camera)]
    frame = [C.POINTER(Motion), C.POINTER(LN.Lens)] + 6 * [i32] + [N.Shard]
    L.sq_shutter_rays_device.argtypes = [i32] + frame + [vp, i64, vp, vp, vp, vp]
    L.sq_shutter_render_device.argtypes = [vp] + frame + [vp, i64, vp, sz, vp, vp, vp, vp, vp, vp]
    _lib = L
    return L


def check(rc):
    N.checked(rc, lib().sq_shutter_last_error)


def build_id():
    """sq_shutter_build_id(): hash of the sources and flags the loaded library was built from (build.py: shutter_source_id)."""
    return lib().sq_shutter_build_id().decode()


def motion_arg(motion):
    """motion as it is; SquiglyError, before any device work, unless it is a Motion the library would take."""
    if not isinstance(motion, Motion):
        raise N.SquiglyError(f"motion must be a Motion, got {type(motion).__name__}")
    t = motion.time_jitter
    if not (0.0 <= t <= 1.0 and math.isfinite(t)):
        raise N.SquiglyError(f"time_jitter must be a number in [0, 1] (got {t!r})")
    return motion


def shutter_rays(ds, motion, lens, samples, subrays, w, h, shard=(None, 0, 1), r_range=None, stream=None):
    """DeviceScene.shutter_rays: lens.lens_rays under a moving camera (sq_shutter_rays_device, dense): (origins, directions, seeds),
    float32 CUDA tensors [nb, rows, h, 3] and int64 [nb, rows, h], nb = r_end - r_begin."""
    import torch
    motion_arg(motion)
    S, R, r0, r1 = LN.frame_args(lens, samples, subrays, r_range)
    sh, rows = P.shard_rows(int(w), shard)
    LN._size_check(rows, h, r1 - r0)
    dev, st = P.call_stream(ds.device, stream)
    with torch.cuda.stream(st):
        o = torch.empty((r1 - r0, rows, h, 3), dtype=torch.float32, device=dev)
        d = torch.empty((r1 - r0, rows, h, 3), dtype=torch.float32, device=dev)
        sd = torch.empty((r1 - r0, rows, h), dtype=torch.int64, device=dev)
    check(lib().sq_shutter_rays_device(ds.device, C.byref(motion), C.byref(lens), S, R, r0, r1, int(w), int(h), sh, None, 0, o.data_ptr(),
                                       d.data_ptr(), sd.data_ptr(), P.stream_ptr(st)))
    return o, d, sd


def render_shutter(ds, motion, lens, samples, subrays, w, h, shard=(None, 0, 1), r_range=None, sums=None, want_sum2=False, want_avg=True,
                   want_rgb=True, work_mb=LN.DEFAULT_WORK_MB, stream=None):
    """DeviceScene.render_shutter: lens.render_lens under a moving camera (sq_shutter_render_device, dense); returns
    LensFrame(sum, sum2, avg, rgb), enqueued on `stream`.  Every argument but `motion` is render_lens'."""
    import torch
    motion_arg(motion)
    S, R, r0, r1 = LN.frame_args(lens, samples, subrays, r_range)
    sized = LN.workspace(work_mb)
    sh, rows = P.shard_rows(int(w), shard)
    pixels = LN._size_check(rows, h)
    s1, s2 = sums if isinstance(sums, (tuple, list)) else (sums, None)
    if s1 is None and (r0 > 0 or s2 is not None):
        raise N.SquiglyError("render_shutter needs the sums of the sub-rays [0, r_begin) when r_range starts above 0")
    want_sum2 = bool(want_sum2) or s2 is not None
    if want_sum2 and s2 is None and r0 > 0:
        raise N.SquiglyError("render_shutter needs sums = (sum, sum2) to carry second moments on from r_begin > 0")
    dev, st = P.call_stream(ds.device, stream)
    for name, t in (("sums", s1), ("sums2", s2)):
        if t is not None:
            P.tensor(name, t, (rows, h, 3), torch.float32, dev)
    nbytes = sized(pixels, r1 - r0)
    with torch.cuda.stream(st):      # outputs and workspace are allocated (and the workspace freed) in the order of the call's stream
        if s1 is None:
            s1 = torch.empty((rows, h, 3), dtype=torch.float32, device=dev)
        if want_sum2 and s2 is None:
            s2 = torch.empty((rows, h, 3), dtype=torch.float32, device=dev)
        avg = torch.empty((rows, h, 3), dtype=torch.float32, device=dev) if want_avg else None
        rgb = torch.empty((rows, h, 3), dtype=torch.uint8, device=dev) if want_rgb else None
        work = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        check(lib().sq_shutter_render_device(ds._h, C.byref(motion), C.byref(lens), S, R, r0, r1, int(w), int(h), sh, None, 0, work.data_ptr(),
                                             nbytes, s1.data_ptr(), P.ptr(s2), None, P.ptr(avg), P.ptr(rgb), P.stream_ptr(st)))
    return LN.LensFrame(s1, s2, avg, rgb)


def render_shutter_masked(ds, motion, lens, samples, subrays, w, h, r_begin, r_end, sums, index, n_live, sums2=None, counts=None,
                          shard=(None, 0, 1), work_mb=LN.DEFAULT_WORK_MB, out_avg=None, out_rgb=None, stream=None):
    """DeviceScene.render_shutter_masked: mlens.render_lens_masked under a moving camera (sq_shutter_render_device with a list);
    returns (out_avg, out_rgb) as given.  Every argument but `motion` is render_lens_masked's; the list is live_pixels'."""
    import torch
    motion_arg(motion)
    S, R, r0, r1 = LN.frame_args(lens, samples, subrays, (r_begin, r_end))
    sized = LN.workspace(work_mb)
    sh, rows = P.shard_rows(int(w), shard)
    pixels = LN._size_check(rows, h)
    L = LN._int("n_live", n_live)
    if L < 0 or L > pixels:
        raise N.SquiglyError(f"n_live must be between 0 and the frame's {pixels} pixels (got {L})")
    if sums is None:
        raise N.SquiglyError("render_shutter_masked needs a sums tensor")
    dev, st = P.call_stream(ds.device, stream)
    for name, t, shape, dtype in (("sums", sums, (rows, h, 3), torch.float32), ("sums2", sums2, (rows, h, 3), torch.float32),
                                  ("counts", counts, (rows, h), torch.int32), ("out_avg", out_avg, (rows, h, 3), torch.float32),
                                  ("out_rgb", out_rgb, (rows, h, 3), torch.uint8)):
        if t is not None:
            P.tensor(name, t, shape, dtype, dev)
    if (not isinstance(index, torch.Tensor) or index.dtype != torch.int32 or index.dim() != 1 or not index.is_contiguous()
            or index.device != dev or index.numel() < L):
        raise N.SquiglyError(f"index must be a contiguous torch.int32 tensor of at least n_live = {L} entries on {dev}")
    if L == 0:
        return out_avg, out_rgb
    nbytes = sized(L, r1 - r0)
    with torch.cuda.stream(st):      # the workspace is allocated (and freed) in the order of the call's stream
        work = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        check(lib().sq_shutter_render_device(ds._h, C.byref(motion), C.byref(lens), S, R, r0, r1, int(w), int(h), sh, index.data_ptr(), L,
                                             work.data_ptr(), nbytes, sums.data_ptr(), P.ptr(sums2), P.ptr(counts), P.ptr(out_avg),
                                             P.ptr(out_rgb), P.stream_ptr(st)))
    return out_avg, out_rgb
