"""The rules every feature of the Python layer follows, each written once: which stream a call runs on, what a
tensor handed to the library must be, how rays and shard tuples come in.  device.py and denoise.py take them from here.

torch is imported where it is used, so that the package imports without it (only the resident-scene path and the denoiser need it).
"""
import ctypes as C

import numpy as np

from . import _native as N


def is_integer(v):
    """The rule for an argument that must be an integer: an int or a numpy integer; a bool and a float, integral or not, are neither."""
    return not isinstance(v, bool) and isinstance(v, (int, np.integer))


def call_stream(device, stream):
    """(torch.device, stream) of a call on `device` (an index or a torch.device): the stream given, else the device's current one.
    Whatever the call allocates it allocates under `with torch.cuda.stream(st)`, in the order of that stream: a block that another
    stream still has work on is not taken."""
    import torch
    dev = device if isinstance(device, torch.device) else torch.device("cuda", int(device))
    return dev, (stream if stream is not None else torch.cuda.current_stream(dev))


def stream_ptr(st):
    """The hipStream_t of a torch stream, as the C-ABI takes it."""
    return C.c_void_p(st.cuda_stream)


def ptr(t):
    """The address of a tensor; None (NULL) for None."""
    return t.data_ptr() if t is not None else None


def tensor(name, t, shape, dtype, dev, says=None):
    """t if it is a contiguous `dtype` tensor of `shape` on `dev`; SquiglyError otherwise, for a thing that is no tensor too.
    says: how the message spells the dtype.  render_rows_range and render_views have said "float32" from their first day and every
    later call "torch.float32"; a message is part of what a caller sees, so each keeps its spelling (None: str(dtype))."""
    import torch
    if (not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape) or t.dtype != dtype or not t.is_contiguous()
            or t.device != dev):
        got = f"{t.dtype} {tuple(t.shape)} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise N.SquiglyError(f"{name} must be a contiguous {says or dtype} tensor of shape {tuple(shape)} on {dev}, got {got}")
    return t


def rays_in(dev, *arrays):
    """A query's origins and directions (numpy, CPU or CUDA tensors, lists) as contiguous float32 tensors on `dev`; float64 is
    rounded to the nearest float32.  Call it under the call's stream: what it allocates is a temporary of that call."""
    import torch
    return tuple(torch.as_tensor(a, device=dev).to(torch.float32).contiguous() for a in arrays)


def shard_ints(w, shard):
    """(row_block, shard_index, n_shards) of a shard tuple as ints; row_block None = all w rows in one block."""
    rb, si, ns = shard
    return int(w if rb is None else rb), int(si), int(ns)


def shard_rows(w, shard):
    """(N.Shard, its row count) of a shard tuple of a w-row image (sq_shard_rows); SquiglyError for a shard that does not exist."""
    sh = N.Shard(*shard_ints(w, shard))
    rows = N.lib().sq_shard_rows(w, sh)
    if rows < 0:
        raise N.SquiglyError(f"bad shard {shard}")
    return sh, rows
