"""ctypes binding of libsquigly_mlens.so (include/squigly_mlens.h): the lens frame of lens.py for the live pixels of a mask only.

A masked lens step lists the live pixels on the device (live_pixels), then gives each listed pixel its next sub-rays and folds them
into the pixel's sum, sum2 and sub-ray count (render_lens_masked); a dead pixel costs no ray.  PyTorch is the plumbing (device
memory, streams); the list, the rays and the fold come from the HIP kernels of csrc/sq_mlens.hip and every sample from
libsquigly_hip.so's radiance query.  There is no fallback: a missing library raises.
"""
import ctypes as C

from . import _native as N
from . import _plumbing as P
from . import lens as LN

# include/squigly_mlens.h
EXPORTED_SYMBOLS = ["sq_mlens_last_error", "sq_mlens_build_id", "sq_mlens_live_device", "sq_mlens_rays_device", "sq_mlens_fold_device",
                    "sq_mlens_render_device"]


def _declare(L):
    vp, i32, i64, sz = C.c_void_p, C.c_int32, C.c_int64, C.c_size_t
    frame = LN.FRAME_ARGTYPES
    L.sq_mlens_live_device.argtypes = [i32, i64, i32, vp, vp, vp, vp, vp]
    L.sq_mlens_rays_device.argtypes = [i32] + frame + [vp, i64, vp, vp, vp, vp]
    L.sq_mlens_fold_device.argtypes = [i32, i64, i32, i32, i32, i32, vp, i64, vp, vp, vp, vp, vp, vp, vp]
    L.sq_mlens_render_device.argtypes = [vp] + frame + [vp, i64, vp, sz, vp, vp, vp, vp, vp, vp]


# SQ_MLENS_LIB_PATH: development aid, loads an experimental build of the same library (build.py: compile_lib(LIBS["mlens"], out=...))
_B = N.Binding("libsquigly_mlens.so", "sq_mlens_", _declare, env="SQ_MLENS_LIB_PATH", client=True)
LIB_PATH, lib, check, build_id = _B
_RENDER = _B.entry("sq_mlens_render_device")


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
                       shard=(None, 0, 1), work_mb=None, out_avg=None, out_rgb=None, stream=None):
    """DeviceScene.render_lens_masked: the sub-rays [r_begin, r_end) of the lens frame for the first n_live pixels of the list
    `index` (sq_mlens_render_device); returns (out_avg, out_rgb) as given.

    sums (required), sums2, counts, out_avg, out_rgb: the frame's [rows, h(, 3)] tensors as in render_rows_masked, updated in place
    for the listed pixels only; counts are SUB-RAYS, and avg = (1 / (r_end * samples / subrays)) * sum.  index: int32 CUDA tensor,
    strictly ascending in its first n_live entries (live_pixels); n_live: an int from the host.  work_mb: as in render_lens, over
    the listed pixels.  Runs under the scene's depth and sky."""
    return LN.frame_listed(_RENDER, "render_lens_masked", cam, ds, lens, samples, subrays, w, h, r_begin, r_end, sums, index, n_live, sums2,
                           counts, shard, work_mb, out_avg, out_rgb, stream)
