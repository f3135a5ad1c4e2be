"""ctypes binding of libsquigly_mlens.so (include/squigly_mlens.h): the lens frame of lens.py for the live pixels of a mask only.

A masked lens step lists the live pixels on the device (live_pixels), then gives each listed pixel its next sub-rays and folds them
into the pixel's sum, sum2 and sub-ray count (render_lens_masked); a dead pixel costs no ray.  PyTorch is the plumbing (device
memory, streams); the list, the rays and the fold come from the HIP kernels of csrc/sq_mlens.hip and every sample from
libsquigly_hip.so's radiance query.  There is no fallback: a missing library raises.
"""
import ctypes as C
import os

from . import _native as N
from . import _plumbing as P
from . import lens as LN

_HERE = os.path.dirname(os.path.abspath(__file__))
# SQ_MLENS_LIB_PATH: development aid, loads an experimental build of the same library (build.py: build_mlens(out=...))
LIB_PATH = os.environ.get("SQ_MLENS_LIB_PATH") or os.path.join(_HERE, "libsquigly_mlens.so")

# include/squigly_mlens.h
EXPORTED_SYMBOLS = ["sq_mlens_last_error", "sq_mlens_build_id", "sq_mlens_live_device", "sq_mlens_rays_device", "sq_mlens_fold_device",
                    "sq_mlens_render_device"]

_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    N.lib()                                   # the library it is a client of, loaded from this package first
    L = N.load(LIB_PATH)
    vp, i32, i64, sz = C.c_void_p, C.c_int32, C.c_int64, C.c_size_t
    L.sq_mlens_last_error.restype = C.c_char_p
    L.sq_mlens_build_id.restype = C.c_char_p
    frame = LN.FRAME_ARGTYPES
    L.sq_mlens_live_device.argtypes = [i32, i64, i32, vp, vp, vp, vp, vp]
    L.sq_mlens_rays_device.argtypes = [i32] + frame + [vp, i64, vp, vp, vp, vp]
    L.sq_mlens_fold_device.argtypes = [i32, i64, i32, i32, i32, i32, vp, i64, vp, vp, vp, vp, vp, vp, vp]
    L.sq_mlens_render_device.argtypes = [vp] + frame + [vp, i64, vp, sz, vp, vp, vp, vp, vp, vp]
    _lib = L
    return L


def check(rc):
    N.checked(rc, lib().sq_mlens_last_error)


def build_id():
    """sq_mlens_build_id(): hash of the sources and flags the loaded library was built from (build.py: mlens_source_id)."""
    return lib().sq_mlens_build_id().decode()


def live_pixels(ds, mask, counts, r_begin, stream=None):
    """DeviceScene.live_pixels: the live list of a masked lens step (sq_mlens_live_device) as (index, n_live): an int32 CUDA tensor
    of as many entries as the frame has pixels, whose first n_live entries are the live pixels (row-major) in ascending order, and
    an int32 CUDA tensor [1] holding n_live.  Only enqueues: read n_live (int(n_live.item()) waits for the stream) before
    render_lens_masked, which takes it from the host.

    mask: uint8 CUDA tensor [rows, h] (None = every pixel); counts: int32 [rows, h] of sub-rays folded (None = no gap guard).  A
    pixel is live iff its mask byte is not 0 and, when r_begin > 0 and counts is given, counts[pixel] == r_begin."""
    import torch
    r0 = LN._int("r_begin", r_begin)
    if r0 < 0 or r0 >= 2 ** 31:
        raise N.SquiglyError(f"r_begin must be at least 0 (got {r0})")
    if mask is None and counts is None:
        raise N.SquiglyError("live_pixels needs a mask or the counts: they give the frame its shape")
    ref = mask if mask is not None else counts
    if not isinstance(ref, torch.Tensor) or ref.dim() != 2:
        raise N.SquiglyError("mask and counts must be CUDA tensors of shape [rows, h]")
    shape = tuple(ref.shape)
    dev, st = P.call_stream(ds.device, stream)
    if mask is not None:
        P.tensor("mask", mask, shape, torch.uint8, dev)
    if counts is not None:
        P.tensor("counts", counts, shape, torch.int32, dev)
    pixels = LN._size_check(shape[0], shape[1])
    with torch.cuda.stream(st):
        index = torch.empty(pixels, dtype=torch.int32, device=dev)
        n_live = torch.zeros(1, dtype=torch.int32, device=dev)
        if pixels:
            check(lib().sq_mlens_live_device(ds.device, pixels, r0, P.ptr(mask), P.ptr(counts), index.data_ptr(), n_live.data_ptr(),
                                             P.stream_ptr(st)))
    return index, n_live


def render_lens_masked(ds, cam, lens, samples, subrays, w, h, r_begin, r_end, sums, index, n_live, sums2=None, counts=None,
                       shard=(None, 0, 1), work_mb=LN.DEFAULT_WORK_MB, out_avg=None, out_rgb=None, stream=None):
    """DeviceScene.render_lens_masked: the sub-rays [r_begin, r_end) of the lens frame for the first n_live pixels of the list
    `index` (sq_mlens_render_device); returns (out_avg, out_rgb) as given.

    sums (required), sums2, counts, out_avg, out_rgb: the frame's [rows, h(, 3)] tensors as in render_rows_masked, updated in place
    for the listed pixels only; counts are SUB-RAYS, and avg = (1 / (r_end * samples / subrays)) * sum.  index: int32 CUDA tensor,
    strictly ascending in its first n_live entries (live_pixels); n_live: an int from the host.  work_mb: as in render_lens, over
    the listed pixels.  Runs under the scene's depth and sky."""
    import torch
    S, R, r0, r1 = LN.frame_args(lens, samples, subrays, (r_begin, r_end))
    sized = LN.workspace(work_mb)
    sh, rows = P.shard_rows(int(w), shard)
    pixels = LN._size_check(rows, h)
    L = LN._int("n_live", n_live)
    if L < 0 or L > pixels:
        raise N.SquiglyError(f"n_live must be between 0 and the frame's {pixels} pixels (got {L})")
    if sums is None:
        raise N.SquiglyError("render_lens_masked needs a sums tensor")
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
        check(lib().sq_mlens_render_device(ds._h, C.byref(cam), C.byref(lens), S, R, r0, r1, int(w), int(h), sh, index.data_ptr(), L,
                                           work.data_ptr(), nbytes, sums.data_ptr(), P.ptr(sums2), P.ptr(counts), P.ptr(out_avg),
                                           P.ptr(out_rgb), P.stream_ptr(st)))
    return out_avg, out_rgb
