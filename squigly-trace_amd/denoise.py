"""ctypes binding of libsquigly_denoise.so (include/squigly_denoise.h) and the helpers around it.

The filter maps device images to device images: colour and (optionally) the variance of its luminance in, guided by the first
hit's triangle id, normal and point (DeviceScene.guides).  PyTorch is the plumbing (device memory, streams); every filtered pixel
comes from the HIP kernels of csrc/sq_denoise.hip.  There is no fallback: a missing library raises.

Sparse frames live here too (sparse_mask, upsample, lattice_offset): under the same guides, which pixels of a frame have to be traced
-- a lattice and the holes -- and every other pixel from its traced neighbours on the same surface.

So does the glare stage (glare, glare_work_bytes, make_glare_params): exposure, white balance and a bloom pyramid over a float frame,
ahead of film.develop.
"""
import collections
import ctypes as C

from . import _native as N
from . import _plumbing as P

# include/squigly_denoise.h; sq_denoise_last_error and the functions a caller uses
EXPORTED_SYMBOLS = ["sq_denoise_last_error", "sq_denoise_build_id", "sq_denoise_pass_form", "sq_denoise_workspace_bytes",
                    "sq_denoise_variance_device", "sq_denoise_device", "sq_denoise_stage_device",
                    "sq_denoise_sparse_mask_device", "sq_denoise_upsample_device",
                    "sq_denoise_glare_work_bytes", "sq_denoise_glare_device"]

FORMS = {"auto": 0, "direct": 1, "tiled": 2}          # params.form (SQ_DENOISE_FORM_*)
# The prototype's parameters.  sigma_p has no default here: it is a length of the scene (denoise_frame derives it).
DEFAULTS = {"passes": 5, "sigma_l": 4.0, "eps_l": 1e-3, "normal_squarings": 3, "form": 0}

Guides = collections.namedtuple("Guides", ["tri", "point", "normal", "surf", "emit"])
Guides.__doc__ = """DeviceScene.guides: per pixel the first hit's triangle (int32, -1 = none), point, unit normal, and its material's surf
and emissive *^ emit (float32 [rows, h, 3]; zeros where nothing is hit)."""


class Params(C.Structure):
    """sq_denoise_params."""
    _fields_ = [("passes", C.c_int32), ("sigma_l", C.c_float), ("eps_l", C.c_float), ("sigma_p", C.c_float),
                ("normal_squarings", C.c_int32), ("form", C.c_int32)]


class SparseParams(C.Structure):
    """sq_denoise_sparse_params."""
    _fields_ = [("sigma_p", C.c_float), ("cos_n", C.c_float)]


class GlareParams(C.Structure):
    """sq_denoise_glare_params."""
    _fields_ = [("exposure", C.c_float), ("gain", C.c_float * 3), ("threshold", C.c_float), ("ceiling", C.c_float), ("levels", C.c_int32),
                ("spread", C.c_float), ("strength", C.c_float), ("form", C.c_int32)]


MAX_GLARE_LEVELS = 8
GLARE_DEFAULTS = {"threshold": 1.0, "ceiling": 16.0, "levels": 5, "spread": 0.5, "strength": 0.1}
MAX_STRIDE = 16               # of a sparse frame's lattice
SPARSE_COS_N = 0.9            # the temporal stage's


def _declare(L):
    vp, i32 = C.c_void_p, C.c_int32
    L.sq_denoise_sparse_mask_device.argtypes = [i32] * 6 + [vp, vp, vp, C.POINTER(SparseParams), vp, vp]
    L.sq_denoise_upsample_device.argtypes = [i32] * 6 + [vp] * 6 + [C.POINTER(SparseParams), vp, vp, vp]
    L.sq_denoise_glare_work_bytes.argtypes = [i32, i32, i32]
    L.sq_denoise_glare_work_bytes.restype = C.c_size_t
    L.sq_denoise_glare_device.argtypes = [i32, i32, i32, vp, vp, C.POINTER(GlareParams), vp, vp, C.c_size_t, vp]
    L.sq_denoise_pass_form.argtypes = [i32]
    L.sq_denoise_pass_form.restype = i32
    L.sq_denoise_workspace_bytes.argtypes = [i32, i32]
    L.sq_denoise_workspace_bytes.restype = C.c_size_t
    L.sq_denoise_variance_device.argtypes = [i32, C.c_int64, vp, vp, vp, vp, vp]
    call = [i32, i32, i32, vp, vp, vp, vp, vp, C.POINTER(Params), vp, vp, vp, C.c_size_t, vp]
    L.sq_denoise_device.argtypes = call
    L.sq_denoise_stage_device.argtypes = call + [i32]


LIB_PATH, lib, check, build_id = N.Binding("libsquigly_denoise.so", "sq_denoise_", _declare)


def workspace_bytes(rows, cols):
    return int(lib().sq_denoise_workspace_bytes(int(rows), int(cols)))


def make_params(sigma_p=None, **kw):
    """sq_denoise_params from keyword arguments: DEFAULTS, sigma_p required; form by number or by name (FORMS)."""
    unknown = set(kw) - set(DEFAULTS)
    if unknown:
        raise N.SquiglyError(f"unknown denoise parameter(s) {sorted(unknown)}: expected sigma_p and any of {sorted(DEFAULTS)}")
    if sigma_p is None:
        raise N.SquiglyError("sigma_p is required: the plane-distance stop in world units (denoise_frame derives it from the scene)")
    p = dict(DEFAULTS, **kw)
    form = p["form"]
    if isinstance(form, str):
        if form not in FORMS:
            raise N.SquiglyError(f"form must be one of {sorted(FORMS)} or a number, got {form!r}")
        form = FORMS[form]
    return Params(int(p["passes"]), float(p["sigma_l"]), float(p["eps_l"]), float(sigma_p), int(p["normal_squarings"]), int(form))


def denoise(color, tri, normal, point, var=None, out=None, stream=None, **params):
    """sq_denoise_device on device tensors; returns (out, out_var), out_var None without var.  Enqueued on `stream`.

    color, normal, point: float32 [rows, cols, 3]; tri: int32 [rows, cols] (a pixel is filtered iff tri >= 0); var: float32
    [rows, cols] or None.  out: a colour tensor, or (colour, variance) tensors, to receive the result (None = allocate); out may
    be color itself, and the variance var itself.  params: sigma_p (required) and any of DEFAULTS.  The workspace is a tensor
    allocated under the stream and handed back to the allocator, in the stream's order, when the call returns."""
    import torch
    if not isinstance(color, torch.Tensor) or color.dim() != 3 or color.shape[-1] != 3 or not color.is_cuda:
        raise N.SquiglyError("color must be a float32 CUDA tensor of shape [rows, cols, 3]")
    dev = color.device
    rows, cols = int(color.shape[0]), int(color.shape[1])
    par = make_params(**params)
    f32 = torch.float32
    P.tensor("color", color, (rows, cols, 3), f32, dev)
    P.tensor("tri", tri, (rows, cols), torch.int32, dev)
    P.tensor("normal", normal, (rows, cols, 3), f32, dev)
    P.tensor("point", point, (rows, cols, 3), f32, dev)
    if var is not None:
        P.tensor("var", var, (rows, cols), f32, dev)
    out_c, out_v = out if isinstance(out, (tuple, list)) else (out, None)
    if out_c is not None:
        P.tensor("out", out_c, (rows, cols, 3), f32, dev)
    if out_v is not None:
        if var is None:
            raise N.SquiglyError("an output variance needs var")
        P.tensor("out variance", out_v, (rows, cols), f32, dev)
    need = workspace_bytes(rows, cols)
    if rows >= 1 and cols >= 1 and need == 0:
        raise N.SquiglyError(f"{rows} x {cols} pixels exceed 2^31 - 1 pixels in one call")
    _, st = P.call_stream(dev, stream)
    with torch.cuda.stream(st):      # outputs and workspace are allocated (and the workspace freed) in the order of the call's stream
        if out_c is None:
            out_c = torch.empty((rows, cols, 3), dtype=f32, device=dev)
        if out_v is None and var is not None:
            out_v = torch.empty((rows, cols), dtype=f32, device=dev)
        work = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
        check(lib().sq_denoise_device(dev.index or 0, rows, cols, color.data_ptr(), P.ptr(var), tri.data_ptr(), normal.data_ptr(),
                                      point.data_ptr(), C.byref(par), out_c.data_ptr(), P.ptr(out_v), work.data_ptr(), need,
                                      P.stream_ptr(st)))
    return out_c, out_v


def denoise_variance(sums, sums2, counts, stream=None):
    """sq_denoise_variance_device: the variance of the pixel mean's luminance, float32 [...], from a masked call's statistics
    (Adaptive.sums, .sums2 float32 [..., 3] and .counts int32 [...])."""
    import torch
    if not isinstance(counts, torch.Tensor) or not counts.is_cuda:
        raise N.SquiglyError("counts must be an int32 CUDA tensor")
    dev, shape = counts.device, tuple(counts.shape)
    P.tensor("counts", counts, shape, torch.int32, dev)
    P.tensor("sums", sums, shape + (3,), torch.float32, dev)
    P.tensor("sums2", sums2, shape + (3,), torch.float32, dev)
    _, st = P.call_stream(dev, stream)
    with torch.cuda.stream(st):
        var = torch.empty(shape, dtype=torch.float32, device=dev)
        check(lib().sq_denoise_variance_device(dev.index or 0, counts.numel(), sums.data_ptr(), sums2.data_ptr(), counts.data_ptr(),
                                               var.data_ptr(), P.stream_ptr(st)))
    return var


def stride_arg(stride):
    """The stride of a sparse frame's lattice as an int; ValueError unless it is an integer in 1..MAX_STRIDE."""
    if not P.is_integer(stride) or not 1 <= int(stride) <= MAX_STRIDE:
        raise ValueError(f"stride must be an integer in 1..{MAX_STRIDE}, got {stride!r}")
    return int(stride)


def lattice_args(stride, offset):
    """(s, oy, ox) of a lattice as ints; ValueError unless stride is an integer in 1..MAX_STRIDE and offset a pair of integers in [0, s)."""
    s = stride_arg(stride)
    try:
        oy, ox = offset
    except (TypeError, ValueError):
        raise ValueError(f"offset must be a pair (oy, ox), got {offset!r}")
    if not P.is_integer(oy) or not P.is_integer(ox) or not (0 <= int(oy) < s and 0 <= int(ox) < s):
        raise ValueError(f"offset must be a pair of integers in [0, {s}), got {offset!r}")
    return s, int(oy), int(ox)


def lattice_offset(frame, stride):
    """The offset (oy, ox) of frame `frame` of a sequence at stride s: with j = frame % s^2, oy = j % s and ox = (j // s + j % s) % s.
    Every offset comes up once in s^2 frames, and the row offset changes with every frame: for s = 2 the order is (0, 0), (1, 1),
    (0, 1), (1, 0)."""
    s = stride_arg(stride)
    if not P.is_integer(frame) or int(frame) < 0:
        raise ValueError(f"frame must be a non-negative integer, got {frame!r}")
    j = int(frame) % (s * s)
    return j % s, (j // s + j % s) % s


def _sparse_params(sigma_p, cos_n):
    if sigma_p is None:
        raise N.SquiglyError("sigma_p is required: the plane-distance stop in world units (default_sigma_p of the scene's bounds)")
    return SparseParams(float(sigma_p), float(cos_n))


def _guide_tensors(guides, dev=None):
    """(rows, cols, device) of guides (anything with .tri, .normal, .point), whose three tensors are checked."""
    import torch
    tri = getattr(guides, "tri", None)
    if not isinstance(tri, torch.Tensor) or tri.dim() != 2 or not tri.is_cuda:
        raise N.SquiglyError("guides.tri must be an int32 CUDA tensor of shape [rows, cols]")
    dev = tri.device if dev is None else dev
    rows, cols = int(tri.shape[0]), int(tri.shape[1])
    P.tensor("guides.tri", tri, (rows, cols), torch.int32, dev)
    P.tensor("guides.normal", guides.normal, (rows, cols, 3), torch.float32, dev)
    P.tensor("guides.point", guides.point, (rows, cols, 3), torch.float32, dev)
    return rows, cols, dev


def sparse_mask(guides, stride, offset, sigma_p=None, cos_n=SPARSE_COS_N, stream=None):
    """sq_denoise_sparse_mask_device: the pixels a sparse frame has to trace, a uint8 CUDA tensor [rows, cols] -- 1 on the lattice
    of `stride` and `offset` = (oy, ox) and at the holes (pixels none of whose lattice neighbours lies on their surface), 0 elsewhere.
    guides: anything with .tri, .normal and .point (DeviceScene.guides).  sigma_p is required (default_sigma_p of the scene).  Pass
    the result to DeviceScene.render_rows_masked(mask=) and then, with what that rendered, to upsample.  Enqueued on `stream`."""
    import torch
    s, oy, ox = lattice_args(stride, offset)
    par = _sparse_params(sigma_p, cos_n)
    rows, cols, dev = _guide_tensors(guides)
    _, st = P.call_stream(dev, stream)
    with torch.cuda.stream(st):
        mask = torch.empty((rows, cols), dtype=torch.uint8, device=dev)
        check(lib().sq_denoise_sparse_mask_device(dev.index or 0, rows, cols, s, oy, ox, guides.tri.data_ptr(), guides.normal.data_ptr(),
                                                  guides.point.data_ptr(), C.byref(par), mask.data_ptr(), P.stream_ptr(st)))
    return mask


def upsample(color, guides, mask, stride, offset, var=None, out=None, stream=None, sigma_p=None, cos_n=SPARSE_COS_N):
    """sq_denoise_upsample_device: the frame `color` (float32 [rows, cols, 3], meaningful where mask is set) with every other pixel
    filled in from its lattice neighbours on the same surface; returns (out, out_var), out_var None without var.  mask: what
    sparse_mask returned for the same guides, stride, offset, sigma_p and cos_n.  var: float32 [rows, cols] or None.  out: a colour
    tensor, or (colour, variance) tensors, to receive the result (None = allocate); they overlap no input.  Enqueued on `stream`."""
    import torch
    s, oy, ox = lattice_args(stride, offset)
    par = _sparse_params(sigma_p, cos_n)
    if not isinstance(color, torch.Tensor) or color.dim() != 3 or color.shape[-1] != 3 or not color.is_cuda:
        raise N.SquiglyError("color must be a float32 CUDA tensor of shape [rows, cols, 3]")
    rows, cols, dev = _guide_tensors(guides, color.device)
    f32 = torch.float32
    P.tensor("color", color, (rows, cols, 3), f32, dev)
    P.tensor("mask", mask, (rows, cols), torch.uint8, dev)
    if var is not None:
        P.tensor("var", var, (rows, cols), f32, dev)
    out_c, out_v = out if isinstance(out, (tuple, list)) else (out, None)
    if out_c is not None:
        P.tensor("out", out_c, (rows, cols, 3), f32, dev)
    if out_v is not None:
        if var is None:
            raise N.SquiglyError("an output variance needs var")
        P.tensor("out variance", out_v, (rows, cols), f32, dev)
    _, st = P.call_stream(dev, stream)
    with torch.cuda.stream(st):
        if out_c is None:
            out_c = torch.empty((rows, cols, 3), dtype=f32, device=dev)
        if out_v is None and var is not None:
            out_v = torch.empty((rows, cols), dtype=f32, device=dev)
        check(lib().sq_denoise_upsample_device(dev.index or 0, rows, cols, s, oy, ox, color.data_ptr(), P.ptr(var), guides.tri.data_ptr(),
                                               guides.normal.data_ptr(), guides.point.data_ptr(), mask.data_ptr(), C.byref(par),
                                               out_c.data_ptr(), P.ptr(out_v), P.stream_ptr(st)))
    return out_c, out_v


def glare_work_bytes(rows, cols, levels):
    """sq_denoise_glare_work_bytes: 16 bytes per pixel of the pyramid's levels; 0 for levels 0 and for what the call refuses."""
    return int(lib().sq_denoise_glare_work_bytes(int(rows), int(cols), int(levels)))


def _glare_number(name, v):
    import numpy as np
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise N.SquiglyError(f"{name} must be a number, got {v!r}")
    with np.errstate(over="ignore"):
        return float(np.float32(v))           # as the library will see it: 1e39 is infinite there, and 1 + 1e-9 is 1


def make_glare_params(exposure=1.0, gain=(1.0, 1.0, 1.0), threshold=1.0, ceiling=16.0, levels=5, spread=0.5, strength=0.1, form=0):
    """sq_denoise_glare_params; what the library would refuse of them is refused here, before any device work.  form by number or by
    name (FORMS)."""
    import math
    try:
        g = [_glare_number("gain", v) for v in gain]
    except TypeError:
        g = []
    if len(g) != 3:
        raise N.SquiglyError(f"gain must be three numbers (r, g, b), got {gain!r}")
    t, c = _glare_number("threshold", threshold), _glare_number("ceiling", ceiling)
    if not 0 <= t < math.inf:
        raise N.SquiglyError(f"threshold must be a finite number >= 0, got {threshold!r}")
    if not t < c < math.inf:
        raise N.SquiglyError(f"ceiling must be a finite number > threshold, got {ceiling!r}")
    if not P.is_integer(levels) or not 0 <= int(levels) <= MAX_GLARE_LEVELS:
        raise N.SquiglyError(f"levels must be an integer in 0..{MAX_GLARE_LEVELS}, got {levels!r}")
    s, w = _glare_number("spread", spread), _glare_number("strength", strength)
    if not 0 <= s < math.inf:
        raise N.SquiglyError(f"spread must be a finite number >= 0, got {spread!r}")
    if not 0 <= w < math.inf:
        raise N.SquiglyError(f"strength must be a finite number >= 0, got {strength!r}")
    if isinstance(form, str):
        if form not in FORMS:
            raise N.SquiglyError(f"form must be one of {sorted(FORMS)} or a number, got {form!r}")
        form = FORMS[form]
    if not P.is_integer(form) or not 0 <= int(form) <= 2:
        raise N.SquiglyError(f"form must be one of {sorted(FORMS)} or a number in 0..2, got {form!r}")
    return GlareParams(_glare_number("exposure", exposure), (C.c_float * 3)(*g), t, c, int(levels), s, w, int(form))


def glare(color, exposure=1.0, gain=(1.0, 1.0, 1.0), threshold=1.0, ceiling=16.0, levels=5, spread=0.5, strength=0.1, form=0, out=None,
          work=None, stream=None):
    """sq_denoise_glare_device on device tensors: the frame `color` (float32 [..., cols, 3]; leading dimensions are rows) times
    `exposure` -- a number, or a float32 CUDA tensor of one element (film.expose()) -- and the white balance `gain`, plus `strength`
    times the glare of what is brighter than `threshold`: a float32 tensor of color's shape, which film.develop takes at exposure 1.
    levels = 0: exposure and gain alone.  out: the tensor to receive the result (None = allocate); it may be color itself.  work: a
    uint8 CUDA tensor of at least glare_work_bytes(rows, cols, levels) bytes, 16-byte aligned (None = allocated under the stream and
    handed back in its order).  Enqueued on `stream`."""
    import torch
    if (not isinstance(color, torch.Tensor) or color.dim() < 2 or color.shape[-1] != 3 or color.dtype != torch.float32 or not color.is_cuda
            or not color.is_contiguous()):
        got = f"{color.dtype} {tuple(color.shape)} on {color.device}" if isinstance(color, torch.Tensor) else type(color).__name__
        raise N.SquiglyError(f"color must be a contiguous torch.float32 CUDA tensor of shape [..., cols, 3], got {got}")
    dev, cols = color.device, int(color.shape[-2])
    rows = int(color.numel() // (3 * cols)) if cols else 0
    if rows < 1 or cols < 1:
        raise N.SquiglyError(f"rows and cols must be at least 1 (got {rows} x {cols})")
    if rows * cols > 2 ** 31 - 1:
        raise N.SquiglyError(f"{rows} x {cols} pixels exceed 2^31 - 1 pixels in one call")
    e_t = exposure if isinstance(exposure, torch.Tensor) else None
    if e_t is not None:
        P.tensor("exposure", e_t, (1,), torch.float32, dev)
    par = make_glare_params(1.0 if e_t is not None else exposure, gain, threshold, ceiling, levels, spread, strength, form)
    if out is not None:
        P.tensor("out", out, tuple(color.shape), torch.float32, dev)
    need = glare_work_bytes(rows, cols, par.levels)
    if work is not None:
        if not isinstance(work, torch.Tensor) or work.dim() != 1 or work.dtype != torch.uint8 or work.device != dev or not work.is_contiguous():
            raise N.SquiglyError(f"work must be a contiguous torch.uint8 tensor of at least {need} bytes on {dev}")
        if work.numel() < need:
            raise N.SquiglyError(f"work holds {work.numel()} bytes: {par.levels} levels of a {rows} x {cols} image need {need}")
        if par.levels and work.data_ptr() % 16:
            raise N.SquiglyError("work must be 16-byte aligned")
    _, st = P.call_stream(dev, stream)
    with torch.cuda.stream(st):      # the result and an absent workspace are allocated (and the workspace freed) in the order of the call's stream
        if out is None:
            out = torch.empty(tuple(color.shape), dtype=torch.float32, device=dev)
        if work is None and par.levels:
            work = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
        check(lib().sq_denoise_glare_device(dev.index or 0, rows, cols, color.data_ptr(), P.ptr(e_t), C.byref(par), out.data_ptr(),
                                            P.ptr(work) if par.levels else None, work.numel() if par.levels else 0, P.stream_ptr(st)))
    return out


def default_sigma_p(bounds):
    """The default plane-distance stop of a scene: 0.5 % of the diagonal of its root bounds (lo, hi as six numbers).  On
    data/scene.obj -- the room, 4 x 4 x 4.23 -- that is 0.0353; the filter was prototyped there with 0.05, which is 0.7 % (pass
    sigma_p=0.05 for the prototype's figures)."""
    import math
    b = [float(v) for v in bounds]
    return 0.005 * math.sqrt(sum((b[3 + i] - b[i]) ** 2 for i in range(3)))


def scene_guides(ds, cam, w, h, shard=(None, 0, 1), stream=None):
    """DeviceScene.guides: camera_rays + intersect, then torch gathers from the scene's triangle and material arrays.  The normal
    is the unit normal of Geometry.hs's `normal`, cross (b - a) (c - a) / its norm, in numpy float32 over the packed triangles: tri and point are intersect's, and normal, surf and
    emit are the rows of those tables, which tests/fuzz_lens.py restates from the oracle's triangles and compares bit for bit."""
    import numpy as np
    import torch
    dev, st = P.call_stream(ds.device, stream)
    with torch.cuda.stream(st):
        tables = getattr(ds, "_guide_tables", None)
        if tables is None:        # per triangle: unit normal, surf, emissive *^ emit; one more row of zeros for "no hit"
            t, m = ds.bih.tris, ds.bih.materials
            mat = t["mat"]
            with np.errstate(all="ignore"):                   # (a degenerate triangle's normal is NaN, a huge emissive times emit inf)
                nrm = np.cross(t["v1"] - t["v0"], t["v2"] - t["v0"]).astype(np.float32)
                nrm = nrm / np.sqrt((nrm * nrm).sum(-1, keepdims=True), dtype=np.float32)
                emit = (m["emissive"][mat][:, None] * m["emit"][mat]) if len(m) else np.zeros((len(t), 3), np.float32)
            surf = m["surf"][mat] if len(m) else np.zeros((len(t), 3), np.float32)
            rows = [np.concatenate([np.asarray(a, np.float32).reshape(len(t), 3), np.zeros((1, 3), np.float32)]) for a in (nrm, surf, emit)]
            tables = ds._guide_tables = tuple(torch.from_numpy(np.ascontiguousarray(r)).to(dev) for r in rows)
        hits = ds.intersect(*ds.camera_rays(cam, w, h, shard, stream=st), want_dist=False, stream=st)
        idx = torch.where(hits.tri >= 0, hits.tri, torch.full_like(hits.tri, tables[0].shape[0] - 1)).long()
        normal, surf, emit = (tab[idx].contiguous() for tab in tables)
    return Guides(hits.tri, hits.point, normal, surf, emit)


def demodulated(g, avg, var=None):
    """(x, var, how) of a frame `avg` under its guides g: where a pixel is hit and all of surf is > 0, x = (avg - emit) / surf --
    the light arriving at the first hit, free of the surface's own colour -- and the variance of its luminance divided by l(surf)^2
    (exact for a grey surface, an estimate otherwise; None stays None); elsewhere both are as given.  how: what remodulated needs.
    Call it under the call's stream.  denoise_frame and Temporal.step share it, operation for operation."""
    import torch
    ok = ((g.tri >= 0) & (g.surf > 0).all(-1))[..., None]
    x = torch.where(ok, (avg - g.emit) / torch.where(ok, g.surf, torch.ones_like(g.surf)), avg)
    scale = None
    if var is not None:
        ls = (0.25 * g.surf[..., 0] + 0.5 * g.surf[..., 1]) + 0.25 * g.surf[..., 2]
        scale = torch.where(ok[..., 0], ls * ls, torch.ones_like(ls))
        var = var / scale
    return x, var, (ok, scale)


def remodulated(g, out, out_var, how):
    """(out, out_var) multiplied back: out * surf + emit and out_var * l(surf)^2 where demodulated divided (out_var None stays None)."""
    import torch
    ok, scale = how
    out = torch.where(ok, out * g.surf + g.emit, out)
    if out_var is not None:
        out_var = out_var * scale
    return out, out_var


def denoise_frame(ds, cam, w, h, avg, var=None, shard=(None, 0, 1), demodulate=True, guides=None, stream=None, **params):
    """Filter the frame `avg` (float32 CUDA tensor [rows, h, 3]) of DeviceScene `ds` under its own guides; returns (out, out_var).

    var: the variance of avg's luminance (denoise_variance) or None.  sigma_p defaults to default_sigma_p of the scene's root
    bounds.  demodulate: the reference's shading makes every sample of a hit pixel surf0 * X + emissive0 *^ emit0 (src/Lib.hs:
    127-137), so where all of surf is > 0 the helper filters X = (avg - emit) / surf -- the light arriving at the first hit, free
    of the surface's own colour -- and multiplies back afterwards; the variance goes with it, divided by l(surf)^2 on the way in and
    multiplied on the way out (exact for a grey surface, an estimate otherwise).  guides: what ds.guides(cam, w, h, shard) returned, to reuse it over frames of one camera."""
    import torch
    _, st = P.call_stream(ds.device, stream)
    if "sigma_p" not in params or params["sigma_p"] is None:
        params["sigma_p"] = default_sigma_p(ds.bih.bounds)
    make_params(**params)                    # refused before any device work
    with torch.cuda.stream(st):
        g = guides if guides is not None else scene_guides(ds, cam, w, h, shard, stream=st)
        if not demodulate:
            return denoise(avg, g.tri, g.normal, g.point, var=var, stream=st, **params)
        x, var, how = demodulated(g, avg, var)
        return remodulated(g, *denoise(x, g.tri, g.normal, g.point, var=var, stream=st, **params), how)
