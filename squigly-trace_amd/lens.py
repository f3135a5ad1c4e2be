"""ctypes binding of libsquigly_lens.so (include/squigly_lens.h) and the helpers around it: anti-aliasing and depth of field.

A lens frame gives every pixel R sub-rays -- jittered over the pixel's area, started on a thin lens -- and folds their radiances
back in a fixed order.  PyTorch is the plumbing (device memory, streams); every ray comes from the HIP kernels of csrc/sq_lens.hip
and every sample from libsquigly_hip.so's radiance query.  There is no fallback: a missing library raises.

The three drivers of a lens frame -- frame_rays, frame_dense, frame_listed -- are written here once; mlens.py and shutter.py call
them with their own entry point, the struct their frames begin with (the camera, or a motion) and the name their messages carry.
"""
import collections
import ctypes as C
import math

from . import _native as N
from . import _plumbing as P

# include/squigly_lens.h
EXPORTED_SYMBOLS = ["sq_lens_last_error", "sq_lens_build_id", "sq_lens_work_bytes", "sq_lens_plan", "sq_lens_rays_device",
                    "sq_lens_fold_device", "sq_lens_render_device"]

MAX_INDEX = 2 ** 31 - 1          # pixels of a call and ray slots of a batch (the header's INDEX WIDTHS)
DEFAULT_WORK_MB = 1024

LensFrame = collections.namedtuple("LensFrame", ["sum", "sum2", "avg", "rgb"])
LensFrame.__doc__ = """Results of DeviceScene.render_lens per pixel: the fold of the sub-ray sums, of their squares (None unless asked for),
(1 / samples) * sum and its tonemap; CUDA tensors [rows, h, 3]."""


class Lens(C.Structure):
    """sq_lens: jitter (0..1, the side in pixels of the square a sub-ray's image point is drawn from; 1 = a box filter over the
    pixel, 0 = makeRay's point), aperture (lens radius in world units, 0 = a pinhole) and focus (forward distance of the plane in
    focus; read only when the aperture is open).  SquiglyError for values the library would refuse."""
    _fields_ = [("jitter", C.c_float), ("aperture", C.c_float), ("focus", C.c_float)]

    def __init__(self, jitter=1.0, aperture=0.0, focus=1.0):
        vals = []
        for name, v in (("jitter", jitter), ("aperture", aperture), ("focus", focus)):
            if isinstance(v, bool) or not isinstance(v, (int, float)):
                raise N.SquiglyError(f"{name} must be a number, got {v!r}")
            vals.append(float(v))
        j, a, f = vals
        if not 0.0 <= j <= 1.0:
            raise N.SquiglyError(f"jitter must be a number in [0, 1] (got {j!r})")
        if not (a >= 0.0 and math.isfinite(a)):
            raise N.SquiglyError(f"aperture must be a finite number >= 0 (got {a!r})")
        if a > 0.0 and not (f > 0.0 and math.isfinite(f)):
            raise N.SquiglyError(f"focus must be a finite number > 0 when the aperture is open (got {f!r})")
        super().__init__(j, a, f)

    def __repr__(self):
        return f"Lens(jitter={self.jitter!r}, aperture={self.aperture!r}, focus={self.focus!r})"


# a frame in both lens libraries' calls: cam, lens, S, R, r_begin, r_end, w, h, shard
FRAME_ARGTYPES = [C.POINTER(N.Camera), C.POINTER(Lens)] + 6 * [C.c_int32] + [N.Shard]


def _declare(L):
    vp, i32, i64, sz = C.c_void_p, C.c_int32, C.c_int64, C.c_size_t
    L.sq_lens_work_bytes.argtypes = [i64, i32]
    L.sq_lens_work_bytes.restype = sz
    L.sq_lens_plan.argtypes = [i64, i32, i32, sz, vp, i32]
    L.sq_lens_plan.restype = i32
    frame = FRAME_ARGTYPES
    L.sq_lens_rays_device.argtypes = [i32] + frame + [vp, vp, vp, vp]
    L.sq_lens_fold_device.argtypes = [i32, i64, i32, i32, i32, vp, vp, vp, vp, vp, vp]
    L.sq_lens_render_device.argtypes = [vp] + frame + [vp, sz, vp, vp, vp, vp, vp]


# SQ_LENS_LIB_PATH: development aid, loads an experimental build of the same library (build.py: compile_lib(LIBS["lens"], out=...))
_B = N.Binding("libsquigly_lens.so", "sq_lens_", _declare, env="SQ_LENS_LIB_PATH", client=True)
LIB_PATH, lib, check, build_id = _B
_RAYS, _RENDER = _B.entry("sq_lens_rays_device"), _B.entry("sq_lens_render_device")


def work_bytes(pixels, subrays):
    """sq_lens_work_bytes: the workspace of a batch of `subrays` sub-rays of `pixels` pixels; 0 beyond the index widths."""
    return int(lib().sq_lens_work_bytes(int(pixels), int(subrays)))


def plan(pixels, r_begin, r_end, work_bytes):
    """sq_lens_plan: the batches [(r0, r1), ...] sq_lens_render_device runs the sub-ray range in; SquiglyError as the library says."""
    n = N.checked(lib().sq_lens_plan(int(pixels), int(r_begin), int(r_end), int(work_bytes), None, 0), lib().sq_lens_last_error, count=True)
    out = (C.c_int32 * (2 * n))()
    lib().sq_lens_plan(int(pixels), int(r_begin), int(r_end), int(work_bytes), out, n)
    return [(int(out[2 * i]), int(out[2 * i + 1])) for i in range(n)]


def _int(name, v):
    if not P.is_integer(v):
        raise N.SquiglyError(f"{name} must be an integer, got {v!r}")
    return int(v)


def frame_args(lens, samples, subrays, r_range=None):
    """(samples, subrays, r_begin, r_end) of a lens frame as ints; SquiglyError, before any device work, for what the library
    would refuse: a lens that is no Lens, samples or sub-rays below 1, sub-rays that do not divide the samples, a bad range."""
    if not isinstance(lens, Lens):
        raise N.SquiglyError(f"lens must be a Lens, got {type(lens).__name__}")
    S, R = _int("samples", samples), _int("subrays", subrays)
    if S < 1 or R < 1 or S >= 2 ** 31:
        raise N.SquiglyError(f"samples and subrays must be at least 1 (got samples = {S}, subrays = {R})")
    if S % R:
        raise N.SquiglyError(f"the sub-rays must divide the samples (got samples = {S}, subrays = {R})")
    if r_range is None:
        r0, r1 = 0, R
    else:
        try:
            r0, r1 = r_range
        except (TypeError, ValueError):
            raise N.SquiglyError(f"r_range must be (r_begin, r_end), got {r_range!r}")
        r0, r1 = _int("r_range[0]", r0), _int("r_range[1]", r1)
    if r0 < 0 or r1 <= r0 or r1 > R:
        raise N.SquiglyError(f"bad sub-ray range [{r0}, {r1}) (need 0 <= r_begin < r_end <= subrays = {R})")
    return S, R, r0, r1


def _size_check(rows, h, subrays=1):
    pixels = int(rows) * int(h)
    if pixels > MAX_INDEX:
        raise N.SquiglyError(f"{rows} x {h} pixels exceed 2^31 - 1 pixels in one call")
    if pixels and subrays > MAX_INDEX // pixels:
        raise N.SquiglyError(f"{subrays} sub-rays of {pixels} pixels exceed 2^31 - 1 ray slots in one batch")
    return pixels


def workspace(work_mb):
    """work_mb of the frame calls (None = DEFAULT_WORK_MB: the one place that default is resolved): SquiglyError unless it is a
    number > 0.  Returns sized(pixels, subrays): the bytes of workspace the call hands the library for that many sub-rays of that
    many pixels -- all they need, at most work_mb MiB."""
    if work_mb is None:
        work_mb = DEFAULT_WORK_MB
    if isinstance(work_mb, bool) or not isinstance(work_mb, (int, float)) or not work_mb > 0 or not math.isfinite(work_mb):
        raise N.SquiglyError(f"work_mb must be a number > 0, got {work_mb!r}")
    budget = int(work_mb * 2 ** 20)

    def sized(pixels, subrays):
        need = work_bytes(pixels, subrays) if pixels else 0
        return min(need, budget) if need else budget
    return sized


# ---- the three drivers of a lens frame.  entry: a library's entry point as a checked call (Binding.entry); head: the struct the
# frame's arguments begin with, the camera or a motion (which its caller has held to its own rules first); list_slot: the entry point
# takes a pixel list (and counts), which a dense call leaves empty. ----
def frame_rays(entry, head, ds, lens, samples, subrays, w, h, shard, r_range, stream, list_slot=False):
    """(origins, directions, seeds) of the sub-rays r_range of every pixel of the shard: float32 CUDA tensors [nb, rows, h, 3] and
    int64 [nb, rows, h], nb = r_end - r_begin."""
    import torch
    S, R, r0, r1 = frame_args(lens, samples, subrays, r_range)
    sh, rows = P.shard_rows(int(w), shard)
    _size_check(rows, h, r1 - r0)
    dev, st = P.call_stream(ds.device, stream)
    with torch.cuda.stream(st):
        o = torch.empty((r1 - r0, rows, h, 3), dtype=torch.float32, device=dev)
        d = torch.empty((r1 - r0, rows, h, 3), dtype=torch.float32, device=dev)
        sd = torch.empty((r1 - r0, rows, h), dtype=torch.int64, device=dev)
    entry(ds.device, C.byref(head), C.byref(lens), S, R, r0, r1, int(w), int(h), sh, *((None, 0) if list_slot else ()), o.data_ptr(),
          d.data_ptr(), sd.data_ptr(), P.stream_ptr(st))
    return o, d, sd


def frame_dense(entry, says, head, ds, lens, samples, subrays, w, h, shard, r_range, sums, want_sum2, want_avg, want_rgb, work_mb, stream,
                list_slot=False):
    """The sub-rays r_range (default: all) of the frame for every pixel of the shard; returns LensFrame(sum, sum2, avg, rgb), enqueued
    on `stream`.  says: the method's name in its messages.  The arguments are render_lens'."""
    import torch
    S, R, r0, r1 = frame_args(lens, samples, subrays, r_range)
    sized = workspace(work_mb)
    sh, rows = P.shard_rows(int(w), shard)
    pixels = _size_check(rows, h)
    s1, s2 = sums if isinstance(sums, (tuple, list)) else (sums, None)
    if s1 is None and (r0 > 0 or s2 is not None):
        raise N.SquiglyError(f"{says} needs the sums of the sub-rays [0, r_begin) when r_range starts above 0")
    want_sum2 = bool(want_sum2) or s2 is not None
    if want_sum2 and s2 is None and r0 > 0:
        raise N.SquiglyError(f"{says} needs sums = (sum, sum2) to carry second moments on from r_begin > 0")
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
        entry(ds._h, C.byref(head), C.byref(lens), S, R, r0, r1, int(w), int(h), sh, *((None, 0) if list_slot else ()), work.data_ptr(),
              nbytes, s1.data_ptr(), P.ptr(s2), *((None,) if list_slot else ()), P.ptr(avg), P.ptr(rgb), P.stream_ptr(st))
    return LensFrame(s1, s2, avg, rgb)


def frame_listed(entry, says, head, ds, lens, samples, subrays, w, h, r_begin, r_end, sums, index, n_live, sums2, counts, shard, work_mb,
                 out_avg, out_rgb, stream):
    """The sub-rays [r_begin, r_end) of the frame for the first n_live pixels of the list `index`; returns (out_avg, out_rgb) as
    given.  says: the method's name in its messages.  The arguments are render_lens_masked's."""
    import torch
    S, R, r0, r1 = frame_args(lens, samples, subrays, (r_begin, r_end))
    sized = workspace(work_mb)
    sh, rows = P.shard_rows(int(w), shard)
    pixels = _size_check(rows, h)
    L = _int("n_live", n_live)
    if L < 0 or L > pixels:
        raise N.SquiglyError(f"n_live must be between 0 and the frame's {pixels} pixels (got {L})")
    if sums is None:
        raise N.SquiglyError(f"{says} needs a sums tensor")
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
        entry(ds._h, C.byref(head), C.byref(lens), S, R, r0, r1, int(w), int(h), sh, index.data_ptr(), L, work.data_ptr(), nbytes,
              sums.data_ptr(), P.ptr(sums2), P.ptr(counts), P.ptr(out_avg), P.ptr(out_rgb), P.stream_ptr(st))
    return out_avg, out_rgb


def lens_rays(ds, cam, lens, samples, subrays, w, h, shard=(None, 0, 1), r_range=None, stream=None):
    """DeviceScene.lens_rays: the sub-rays [r_begin, r_end) of every pixel of the shard (sq_lens_rays_device) as (origins,
    directions, seeds): float32 CUDA tensors [nb, rows, h, 3] and int64 [nb, rows, h], nb = r_end - r_begin.  With them
    ds.raytrace(origins, directions, seeds=seeds, samples=samples // subrays) is every sub-ray's sum."""
    return frame_rays(_RAYS, cam, ds, lens, samples, subrays, w, h, shard, r_range, stream)


def render_lens(ds, cam, lens, samples, subrays, w, h, shard=(None, 0, 1), r_range=None, sums=None, want_sum2=False, want_avg=True,
                want_rgb=True, work_mb=None, stream=None):
    """DeviceScene.render_lens: the sub-rays r_range (default: all) of the lens frame (sq_lens_render_device); returns
    LensFrame(sum, sum2, avg, rgb), enqueued on `stream`.

    samples, subrays: S and R of include/squigly_lens.h; R divides S and S / R samples ride on each sub-ray.  sums: the fold so far
    -- a float32 CUDA tensor [rows, h, 3], or a pair (sum, sum2) of them -- required when r_range starts above 0, updated in place,
    allocated otherwise.  want_sum2: also fold the squares of the sub-ray sums (implied by a pair).  avg = (1 / samples) * sum of
    the sub-rays folded so far and rgb its tonemap (None unless wanted).  work_mb: the most workspace, in MiB, the call allocates
    (a tensor under the stream, handed back when the call returns; None = DEFAULT_WORK_MB): the frame runs in batches of as many
    whole sub-rays as fit, and its bits do not depend on that.  Runs under the scene's depth and sky."""
    return frame_dense(_RENDER, "render_lens", cam, ds, lens, samples, subrays, w, h, shard, r_range, sums, want_sum2, want_avg, want_rgb,
                       work_mb, stream)
