"""ctypes binding of libsquigly_temporal.so (include/squigly_temporal.h) and the driver around it.

The library accumulates a sequence of frames under a moving camera: every frame's colour and variance are blended with what the
previous frame's history holds at the place the pixel's first hit was seen from the previous camera.  PyTorch is the plumbing (device
memory, streams); every accumulated pixel comes from the HIP kernel of csrc/sq_temporal.hip.  There is no fallback: a missing library
raises.
"""
import collections
import ctypes as C

from . import _native as N
from . import _plumbing as P

# include/squigly_temporal.h
EXPORTED_SYMBOLS = ["sq_temporal_last_error", "sq_temporal_build_id", "sq_temporal_history_bytes", "sq_temporal_project",
                    "sq_temporal_accumulate_device", "sq_temporal_accumulate_moving_device", "sq_temporal_unpack_device"]

# sigma_p has no default here: it is a length of the scene (Temporal takes denoise.default_sigma_p of it).
DEFAULTS = {"alpha_min": 0.1, "max_history": 32, "cos_n": 0.9}

History = collections.namedtuple("History", ["color", "var", "len", "tri", "normal", "point"])
History.__doc__ = """A history block as plain images (unpack): the accumulated colour [rows, cols, 3] and variance [rows, cols], the
history length (int32), and the guides of the frame that wrote it: triangle (int32), unit normal and point."""


class Params(C.Structure):
    """sq_temporal_params."""
    _fields_ = [("alpha_min", C.c_float), ("max_history", C.c_int32), ("sigma_p", C.c_float), ("cos_n", C.c_float)]


class Clamp(C.Structure):
    """sq_temporal_clamp."""
    _fields_ = [("radius", C.c_int32), ("k", C.c_float)]


FORMS = {"auto": 0, "direct": 1, "tiled": 2}            # SQ_TEMPORAL_FORM_*: how the clamp's window is read; the bits are the same
FLAG_BLENDED, FLAG_CLAMPED, FLAG_MOVED = 1, 2, 4        # SQ_TEMPORAL_FLAG_*
CLAMP_RADIUS = 1                                        # of a clamp given as a number: the 3 x 3 window


def _declare(L):
    vp, i32 = C.c_void_p, C.c_int32
    L.sq_temporal_history_bytes.argtypes = [i32, i32]
    L.sq_temporal_history_bytes.restype = C.c_size_t
    L.sq_temporal_project.argtypes = [C.POINTER(N.Camera), i32, i32, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.sq_temporal_accumulate_device.argtypes = [i32, i32, i32, vp, vp, vp, vp, vp, vp, C.POINTER(N.Camera), vp, C.POINTER(Params),
                                                vp, vp, vp, vp, vp]
    L.sq_temporal_accumulate_moving_device.argtypes = [i32, i32, i32, vp, vp, vp, vp, vp, vp, C.POINTER(N.Camera), vp, C.POINTER(Params),
                                                       vp, i32, vp, i32, C.POINTER(Clamp), i32, vp, vp, vp, vp, vp, vp]
    L.sq_temporal_unpack_device.argtypes = [i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]


LIB_PATH, lib, check, build_id = N.Binding("libsquigly_temporal.so", "sq_temporal_", _declare)


def history_bytes(rows, cols):
    return int(lib().sq_temporal_history_bytes(int(rows), int(cols)))


def project(prev_cam, w, h, point):
    """sq_temporal_project: (projects, fx, fy) of the world point `point` (three numbers) in the w rows x h columns image of
    prev_cam -- fx the column, fy the row, as Python floats holding the float32 values.  Host code: no device is touched."""
    pt = (C.c_float * 3)(*[float(v) for v in point])
    fx, fy = C.c_float(), C.c_float()
    rc = N.checked(lib().sq_temporal_project(C.byref(prev_cam), int(w), int(h), pt, C.byref(fx), C.byref(fy)),
                   lib().sq_temporal_last_error, count=True)
    return bool(rc), fx.value, fy.value


def make_params(sigma_p=None, **kw):
    """sq_temporal_params from keyword arguments: DEFAULTS, sigma_p required."""
    unknown = set(kw) - set(DEFAULTS)
    if unknown:
        raise N.SquiglyError(f"unknown temporal parameter(s) {sorted(unknown)}: expected sigma_p and any of {sorted(DEFAULTS)}")
    if sigma_p is None:
        raise N.SquiglyError("sigma_p is required: the plane-distance stop in world units (Temporal derives it from the scene)")
    p = dict(DEFAULTS, **kw)
    if not P.is_integer(p["max_history"]):
        raise N.SquiglyError(f"max_history must be an integer in 1..65536, got {p['max_history']!r}")
    return Params(float(p["alpha_min"]), int(p["max_history"]), float(sigma_p), float(p["cos_n"]))


def clamp_arg(clamp):
    """None (off), or the (k, radius) of a clamp given as a number k >= 0 (radius CLAMP_RADIUS) or as a pair (k, radius), radius in
    1..3.  ValueError otherwise."""
    if clamp is None:
        return None
    k, radius = clamp if isinstance(clamp, (tuple, list)) and len(clamp) == 2 else (clamp, CLAMP_RADIUS)
    if isinstance(k, bool) or not isinstance(k, (int, float)) or not float(k) >= 0:
        raise ValueError(f"clamp must be a number k >= 0 or a pair (k, radius), got {clamp!r}")
    if not P.is_integer(radius) or not 1 <= int(radius) <= 3:
        raise ValueError(f"the clamp's radius must be an integer in 1..3, got {radius!r}")
    return float(k), int(radius)


def back_transforms(prev_poses, poses):
    """accumulate's `back` for objects that moved from prev_poses to poses, both [n_objects, 3, 4] arrays [R | t] with
    world = R local + t: per object the row-major 3 x 4 of M_prev M_now^-1, which takes a world point of the current frame to where
    the same surface point was in the previous one.  float32 [n_objects, 12], computed in float64 on the host and rounded once."""
    import numpy as np
    a, b = np.asarray(prev_poses, np.float64), np.asarray(poses, np.float64)
    if a.ndim != 3 or a.shape[1:] != (3, 4) or a.shape != b.shape:
        raise ValueError(f"poses must be two [n_objects, 3, 4] arrays of one shape, got {a.shape} and {b.shape}")
    out = np.empty((len(a), 12), np.float32)
    for i, (mp, mn) in enumerate(zip(a, b)):
        inv = np.linalg.inv(mn[:, :3])
        L = mp[:, :3] @ inv
        out[i] = np.concatenate([L, (mp[:, 3] - L @ mn[:, 3]).reshape(3, 1)], 1).reshape(12)
    return out


def _size(rows, cols):
    need = history_bytes(rows, cols)
    if need == 0:
        raise N.SquiglyError(f"rows and cols must be at least 1 (got {rows} x {cols})" if rows < 1 or cols < 1
                             else f"{rows} x {cols} pixels exceed 2^31 - 1 pixels in one call")
    return need


def history(rows, cols, device):
    """A history block for rows x cols frames on `device` (an index or a torch.device): a uint8 tensor of history_bytes(rows, cols)
    bytes.  Its contents mean nothing until accumulate has written it as nxt."""
    import torch
    dev, _ = P.call_stream(device, None)
    return torch.empty(_size(int(rows), int(cols)), dtype=torch.uint8, device=dev)


_new_block = history          # (Temporal's constructor has an argument of that name)


def _block(name, t, need, dev):
    import torch
    return P.tensor(name, t, (need,), torch.uint8, dev)


def accumulate(color, var, guides, prev_cam, prev, nxt, alpha=None, out=None, stream=None, objects=None, back=None, clamp=None,
               want_flags=False, form="auto", **params):
    """sq_temporal_accumulate_device on device tensors; returns (out, out_var, out_len).  Enqueued on `stream`.
    With any of objects, back, clamp and want_flags it is sq_temporal_accumulate_moving_device: objects (int32 [n_tris], the rigid
    object of every triangle of the current scene; object_table) and back (float32 [n_objects, 12], back_transforms; a host array is
    uploaded on the call's stream) go together; clamp is clamp_arg's (a number k, or (k, radius)); want_flags=True returns
    (out, out_var, out_len, flags) with flags uint8 [rows, cols] of FLAG_BLENDED, FLAG_CLAMPED and FLAG_MOVED; form (one of FORMS)
    forces how the clamp's window is read.  Under a clamp the output colour may not be `color` itself.

    color: float32 [rows, cols, 3]; var: float32 [rows, cols]; guides: anything with .tri (int32 [rows, cols]), .normal and .point
    (float32 [rows, cols, 3]) -- DeviceScene.guides of the frame's camera.  prev_cam, prev: the camera and the block (history()) of
    the previous frame, both None for the first frame.  nxt: the block this frame writes (not prev).  alpha: float32 [rows, cols] or
    None, the least weight of the new frame per pixel.  out: (colour, variance) or (colour, variance, length) tensors to receive
    the result (None = allocate each); the colour may be color itself and the variance var itself.  params: sigma_p (required) and
    any of DEFAULTS."""
    import torch
    if not isinstance(color, torch.Tensor) or color.dim() != 3 or color.shape[-1] != 3 or not color.is_cuda:
        raise N.SquiglyError("color must be a float32 CUDA tensor of shape [rows, cols, 3]")
    dev = color.device
    rows, cols = int(color.shape[0]), int(color.shape[1])
    par = make_params(**params)
    f32 = torch.float32
    P.tensor("color", color, (rows, cols, 3), f32, dev)
    P.tensor("var", var, (rows, cols), f32, dev)
    P.tensor("guides.tri", guides.tri, (rows, cols), torch.int32, dev)
    P.tensor("guides.normal", guides.normal, (rows, cols, 3), f32, dev)
    P.tensor("guides.point", guides.point, (rows, cols, 3), f32, dev)
    if alpha is not None:
        P.tensor("alpha", alpha, (rows, cols), f32, dev)
    need = _size(rows, cols)
    if (prev is None) != (prev_cam is None):
        raise N.SquiglyError("prev and prev_cam go together: both None for the first frame, both given after it")
    if prev is not None:
        _block("prev", prev, need, dev)
    _block("nxt", nxt, need, dev)
    out = tuple(out) if out is not None else ()
    if len(out) > 3:
        raise N.SquiglyError("out must be (colour, variance) or (colour, variance, length)")
    out_c, out_v, out_l = out + (None,) * (3 - len(out))
    if out_c is not None:
        P.tensor("out colour", out_c, (rows, cols, 3), f32, dev)
    if out_v is not None:
        P.tensor("out variance", out_v, (rows, cols), f32, dev)
    if out_l is not None:
        P.tensor("out length", out_l, (rows, cols), torch.int32, dev)
    moving = objects is not None or back is not None or clamp is not None or want_flags
    if (objects is None) != (back is None):
        raise N.SquiglyError("objects and back go together: both None (nothing moves) or both given")
    if form not in FORMS:
        raise N.SquiglyError(f"form must be one of {sorted(FORMS)}, got {form!r}")
    try:
        clamp = clamp_arg(clamp)
    except ValueError as e:
        raise N.SquiglyError(str(e)) from None
    if objects is not None:
        if not isinstance(objects, torch.Tensor) or objects.dim() != 1:
            raise N.SquiglyError("objects must be an int32 CUDA tensor of shape [n_tris]")
        P.tensor("objects", objects, (int(objects.shape[0]),), torch.int32, dev)
        if not isinstance(back, torch.Tensor):
            import numpy as np
            back = torch.from_numpy(np.ascontiguousarray(back, dtype=np.float32))
        if back.dim() != 2 or back.shape[1] != 12:
            raise N.SquiglyError(f"back must be float32 of shape [n_objects, 12], got {tuple(back.shape)}")
        if objects.shape[0] == 0 or back.shape[0] == 0:          # (an empty tensor's address is NULL: say what the library would)
            raise N.SquiglyError("objects is given with n_tris = 0" if objects.shape[0] == 0 else "back is given with n_objects = 0")
    _, st = P.call_stream(dev, stream)
    with torch.cuda.stream(st):      # outputs are allocated in the order of the call's stream
        if out_c is None:
            out_c = torch.empty((rows, cols, 3), dtype=f32, device=dev)
        if out_v is None:
            out_v = torch.empty((rows, cols), dtype=f32, device=dev)
        if out_l is None:
            out_l = torch.empty((rows, cols), dtype=torch.int32, device=dev)
        # what both entry points take, ahead of and behind the moving call's own arguments
        head = (dev.index or 0, rows, cols, color.data_ptr(), var.data_ptr(), guides.tri.data_ptr(), guides.normal.data_ptr(),
                guides.point.data_ptr(), P.ptr(alpha), None if prev_cam is None else C.byref(prev_cam), P.ptr(prev), C.byref(par))
        tail = (nxt.data_ptr(), out_c.data_ptr(), out_v.data_ptr(), out_l.data_ptr())
        if not moving:
            check(lib().sq_temporal_accumulate_device(*head, *tail, P.stream_ptr(st)))
            return out_c, out_v, out_l
        if back is not None and not back.is_cuda:          # through pinned memory: the copy only enqueues, behind the stream's work
            back = back.pin_memory().to(dev, non_blocking=True)
        if back is not None:
            P.tensor("back", back, (int(back.shape[0]), 12), f32, dev)
        flags = torch.empty((rows, cols), dtype=torch.uint8, device=dev) if want_flags else None
        cl = None if clamp is None else Clamp(clamp[1], clamp[0])
        check(lib().sq_temporal_accumulate_moving_device(
            *head, P.ptr(objects), 0 if objects is None else int(objects.shape[0]), P.ptr(back), 0 if back is None else int(back.shape[0]),
            None if cl is None else C.byref(cl), FORMS[form], *tail, P.ptr(flags), P.stream_ptr(st)))
    return (out_c, out_v, out_l, flags) if want_flags else (out_c, out_v, out_l)


def unpack(hist, rows, cols, stream=None):
    """sq_temporal_unpack_device: the History (plain images) of the block `hist` of rows x cols frames.  Enqueued on `stream`."""
    import torch
    if not isinstance(hist, torch.Tensor) or not hist.is_cuda:
        raise N.SquiglyError("hist must be a uint8 CUDA tensor (history())")
    rows, cols = int(rows), int(cols)
    dev = hist.device
    _block("hist", hist, _size(rows, cols), dev)
    _, st = P.call_stream(dev, stream)
    with torch.cuda.stream(st):
        f32, i32 = torch.float32, torch.int32
        h = History(torch.empty((rows, cols, 3), dtype=f32, device=dev), torch.empty((rows, cols), dtype=f32, device=dev),
                    torch.empty((rows, cols), dtype=i32, device=dev), torch.empty((rows, cols), dtype=i32, device=dev),
                    torch.empty((rows, cols, 3), dtype=f32, device=dev), torch.empty((rows, cols, 3), dtype=f32, device=dev))
        check(lib().sq_temporal_unpack_device(dev.index or 0, rows, cols, hist.data_ptr(), h.color.data_ptr(), h.var.data_ptr(),
                                              h.len.data_ptr(), h.tri.data_ptr(), h.normal.data_ptr(), h.point.data_ptr(), P.stream_ptr(st)))
    return h


def alpha_table(ds):
    """Per triangle of the scene the material's `reflective`, and one more entry of 0 for "no hit": a float32 tensor on the
    scene's device, built once per scene.  Gathered by a frame's triangle ids it is accumulate's alpha: the mirror (reflective 1)
    takes no history, a wall of reflective 0.2 keeps a >= 0.2 -- the view-dependent share of a pixel is not reprojected."""
    import numpy as np
    import torch
    table = getattr(ds, "_temporal_alpha", None)
    if table is None:
        t, m = ds.bih.tris, ds.bih.materials
        refl = m["reflective"][t["mat"]] if len(m) else np.zeros(len(t), np.float32)
        refl = np.concatenate([np.asarray(refl, np.float32).reshape(len(t)), np.zeros(1, np.float32)])
        table = ds._temporal_alpha = torch.from_numpy(np.ascontiguousarray(refl)).to(torch.device("cuda", ds.device))
    return table


def object_table(ds):
    """accumulate's `objects` of the scene: per triangle (in ds.bih.tris order, the order of a frame's triangle ids) its material's
    index, an int32 tensor on the scene's device, built once per scene.  The default objects are the materials: a caller who wants
    two objects of one material gives them two material entries."""
    import numpy as np
    import torch
    table = getattr(ds, "_temporal_objects", None)
    if table is None:
        mat = np.ascontiguousarray(ds.bih.tris["mat"], dtype=np.int32)
        table = ds._temporal_objects = torch.from_numpy(mat.copy()).to(torch.device("cuda", ds.device))
    return table


def frame_alpha(ds, tri):
    """accumulate's alpha of a frame whose first hits are `tri` (int32 CUDA tensor; -1 = none): alpha_table gathered by tri."""
    import torch
    table = alpha_table(ds)
    idx = torch.where(tri >= 0, tri, torch.full_like(tri, table.shape[0] - 1)).long()
    return table[idx].contiguous()


def tonemap(avg):
    """rgbFloatToPixelRGB (src/Lib.hs:93-104) in torch float32 operations, on the device and without a host wait: uint8 of avg's
    shape.  A preview: the arctangent is torch's, so the result is not pinned to the bit as the renderer's own tonemap is."""
    import math
    import torch
    hi, lo = avg.amax(-1, keepdim=True), avg.amin(-1, keepdim=True)
    intensity = torch.atan(0.5 * (hi + lo)) / (math.pi / 2)
    s = torch.nan_to_num((intensity / hi) * avg, nan=0.0, posinf=1.0, neginf=0.0)
    return torch.floor(s * 255).clamp_(0, 255).to(torch.uint8)


def _temporal_args(spp, period, alpha_min, max_history):
    """The refusals of Temporal's numbers, before any device work."""
    for name, v in (("spp", spp), ("period", period), ("max_history", max_history)):
        if not P.is_integer(v) or int(v) < 1:
            raise ValueError(f"{name} must be a positive integer, got {v!r}")
    if int(spp) * int(period) > 2 ** 31 - 1:
        raise ValueError(f"spp * period = {int(spp) * int(period)} samples exceed 2^31 - 1")
    if int(max_history) > 65536:
        raise ValueError(f"max_history must be in 1..65536, got {max_history}")
    if isinstance(alpha_min, bool) or not isinstance(alpha_min, (int, float)) or not 0 <= float(alpha_min) <= 1:
        raise ValueError(f"alpha_min must be a number in 0..1, got {alpha_min!r}")


class Temporal:
    """A sequence of frames of one scene under a moving camera, each rendered with `spp` samples and accumulated over the frames
    before it (DeviceScene.render_rows_masked, denoise_variance, DeviceScene.guides, accumulate and, optionally, the filter).

    step(cam) renders frame f = `frames` and returns (avg, var, length, rgb): the accumulated colour [w, h, 3] and the variance of
    its luminance [w, h] (float32), the history length of every pixel (int32) and a tonemapped preview (uint8; tonemap(), or
    film= (a Film): the image it develops on the device, pinned to the bit).  The
    frame's samples are the range [(f mod period) * spp, + spp) of the (spp * period)-sample frame, so that consecutive frames
    take different seeds: with equal seeds a still camera would add nothing.  `noisy` is the frame's own spp-sample mean.
    The history lives in demodulated space (denoise_frame's: X = (avg - emit) / surf where all of surf is > 0), a pixel's alpha is
    its material's `reflective` (alpha_table), and sigma_p defaults to denoise.default_sigma_p of the scene.  denoise: None = off;
    True, a sigma_l or a dict of denoise parameters (render.denoise_options) filters the accumulated colour and variance under the
    same guides before the result is remodulated; the history holds the unfiltered accumulation.
    A checkpoint is (history, camera, frames) -- copy them away and pass them back in as history=, camera=, frames= -- and
    depth, sky as in Progressive (sky=None: a fresh sequence under the scene's own sky).  reset() starts a new sequence.
    sparse (None = every pixel is traced, the calls as they were; S = a stride in 1..16): a sparse frame.  step then takes the guides
    first, traces only the pixels of denoise.sparse_mask at lattice_offset(frames, S) -- the lattice, which moves from frame to frame
    so that every pixel is traced once in S * S frames, and the holes -- and fills the others in from their traced neighbours on the
    same surface (denoise.upsample; sigma_p and cos_n are the accumulation's) after the demodulation and before the accumulation.  A
    traced pixel holds what the dense frame holds there, bit for bit.  `noisy` is then meaningful on the live pixels only, and `live`
    is the frame's mask (uint8 [w, h]; None without sparse).
    Geometry that moves: step(cam, scene=ds_f, back=B) renders the frame from ds_f, the DeviceScene that holds this frame's geometry
    (None = the constructor's), and reprojects through B ([n_objects, 12], back_transforms: the move from the previous step's
    geometry to this one's; None = nothing moved).  The guides, the alpha table, the object table (object_table: a triangle's
    object is its material) and the masked render all come from that scene.  The frame's own state (sums, counts, history blocks)
    depends on the size alone, so it stays the constructor's; a scene given to step is bound for that step only, and must agree
    with what the sequence was begun under -- the device, the count of materials, the depth and the sky, all recorded at
    construction, so that the constructor's scene may be closed once steps bring scenes of their own: SquiglyError for a scene on
    another device, with another count of materials (the objects of `back` would be others), or under another depth or sky.  `back` without as many rows as the scene has materials is
    refused too.  sparse with a scene given to step is refused: the lattice's fill has not been carried through a changing scene.
    clamp (None = off; k or (k, radius), clamp_arg): the history colour is held to mean -/+ k standard deviations of the current
    frame's (2 radius + 1)^2 neighbourhood before it is blended, which answers light that changed on surfaces that did not move
    (a moving object's shadow).  `flags` is the last step's FLAG_* image (uint8 [w, h]) when a clamp or a back was given, else None.
    With scene=None, back=None and clamp=None every call is what it was.
    Whole frames on one device; path-traced frames only."""

    def __init__(self, ds, w, h, spp, period=64, alpha_min=0.1, max_history=32, denoise=None, demodulate=True, depth=None, sky=None,
                 sigma_p=None, cos_n=0.9, history=None, camera=None, frames=0, film=None, sparse=None, clamp=None):
        import torch
        from . import device as D
        from .denoise import default_sigma_p, make_params as denoise_params, stride_arg
        from .render import denoise_arg
        _temporal_args(spp, period, alpha_min, max_history)
        self.sparse = None if sparse is None else stride_arg(sparse)
        from .film import film_arg
        self.film = film_arg(film)
        self.clamp = clamp_arg(clamp)
        if not P.is_integer(frames) or int(frames) < 0:
            raise ValueError(f"frames must be a non-negative integer, got {frames!r}")
        if (history is None) != (camera is None):
            raise ValueError("resuming needs the history and the camera it was written under, a fresh sequence neither")
        self.spp, self.period, self.demodulate = int(spp), int(period), bool(demodulate)
        self.params = dict(alpha_min=float(alpha_min), max_history=int(max_history), cos_n=float(cos_n),
                           sigma_p=default_sigma_p(ds.bih.bounds) if sigma_p is None else float(sigma_p))
        make_params(**self.params)
        self.denoise = denoise_arg(denoise)
        if self.denoise is not None:
            self.denoise.setdefault("sigma_p", self.params["sigma_p"])
            denoise_params(**self.denoise)                       # refused before any device work
        self._frame = D._Frame()
        rows = self._frame._begin(ds, None, self.spp * self.period, w, h, False, (None, 0, 1), depth=depth,
                                  sky=D.SCENE_SKY if sky is None else sky)
        self.ds, self.w, self.h = ds, int(w), int(h)
        self._begun = (ds.device, len(ds.bih.materials))          # what a step's own scene must agree with
        self.depth, self.sky = self._frame.depth, self._frame.sky
        dev = self._dev = torch.device("cuda", ds.device)
        self._sums = torch.zeros((rows, self.h, 3), dtype=torch.float32, device=dev)
        self._sums2 = torch.zeros((rows, self.h, 3), dtype=torch.float32, device=dev)
        self._counts = torch.full((rows, self.h), self.spp, dtype=torch.int32, device=dev)
        self._blocks = [_new_block(rows, self.h, dev), _new_block(rows, self.h, dev)]
        self._cur, self._cam, self.frames, self.noisy, self.live, self.flags = None, None, int(frames), None, None, None
        if history is not None:
            t = torch.as_tensor(history, dtype=torch.uint8, device=dev).contiguous()
            if tuple(t.shape) != tuple(self._blocks[0].shape):
                raise ValueError(f"history must have shape {tuple(self._blocks[0].shape)}, got {tuple(t.shape)}")
            self._blocks[0].copy_(t)
            self._cur, self._cam = 0, N.Camera.from_buffer_copy(bytes(camera))

    history = property(lambda self: None if self._cur is None else self._blocks[self._cur],
                       doc="The block the last step wrote (a uint8 CUDA tensor the next step reads: copy it to keep it), None before the first.")
    camera = property(lambda self: self._cam, doc="The camera of the last step (a copy), None before the first.")

    def reset(self):
        """Forget the history and start a new sequence: the next step is frame 0."""
        self._cur, self._cam, self.frames = None, None, 0

    def forget(self):
        """Forget the history alone: the next frame accumulates nothing, and the frame count goes on."""
        self._cur, self._cam = None, None

    def _bound(self, scene, back):
        """The scene of this step, after the refusals of one that is not the constructor's."""
        from . import device as D
        if scene is None or scene is self.ds:
            ds = self.ds
            self._frame._unchanged()
        else:
            ds = scene
            device, n_materials = self._begun
            if ds.device != device:
                raise N.SquiglyError(f"the sequence runs on device {device}, the step's scene is on device {ds.device}")
            if len(ds.bih.materials) != n_materials:
                raise N.SquiglyError(f"the sequence was begun with {n_materials} materials, the step's scene has "
                                     f"{len(ds.bih.materials)}: the objects of a move are the materials")
            if self.sparse is not None:
                raise N.SquiglyError("sparse frames are not carried through a scene that changes from step to step")
            for name, _, key, mine, theirs, _ in D._UNDER:
                was, have = getattr(self._frame, name), getattr(ds, name)
                if key(have) != key(was):
                    raise N.SquiglyError(f"the frame was begun under {mine(was)}, the step's scene has {theirs(have)}")
        if back is not None and (getattr(back, "ndim", 0) != 2 or tuple(back.shape) != (len(ds.bih.materials), 12)):
            raise N.SquiglyError(f"back must have shape ({len(ds.bih.materials)}, 12): a row per material of the scene, got "
                                 f"{tuple(getattr(back, 'shape', ()))}")
        return ds

    def step(self, cam, stream=None, scene=None, back=None):
        """Render the next frame under `cam` and accumulate it; returns (avg, var, length, rgb).  Enqueued on `stream`.
        scene, back: this frame's geometry and its move from the last step's (the class's docstring)."""
        import torch
        from .denoise import demodulated, denoise, denoise_variance, lattice_offset, remodulated, sparse_mask, upsample
        ds, w, h = self._bound(scene, back), self.w, self.h
        moving = {}
        if back is not None:
            moving.update(objects=object_table(ds), back=back)
        if self.clamp is not None:
            moving.update(clamp=self.clamp)
        if moving:
            moving.update(want_flags=True)
        _, st = P.call_stream(self._dev, stream)
        k0 = (self.frames % self.period) * self.spp
        with torch.cuda.stream(st):
            self._sums.zero_()
            self._sums2.zero_()
            g = live = None
            if self.sparse is not None:                           # the guides first: they say which pixels are traced
                g = ds.guides(cam, w, h, stream=st)
                lattice = dict(stride=self.sparse, offset=lattice_offset(self.frames, self.sparse), sigma_p=self.params["sigma_p"],
                               cos_n=self.params["cos_n"])
                live = sparse_mask(g, stream=st, **lattice)
            ds.render_rows_masked(cam, self.spp * self.period, w, h, k0, k0 + self.spp, self._sums, mask=live, sums2=self._sums2,
                                  want_avg=False, want_rgb=False, stream=st)
            noisy = self._sums / float(self.spp)
            var = denoise_variance(self._sums, self._sums2, self._counts, stream=st)
            if g is None:
                g = ds.guides(cam, w, h, stream=st)
            x, how = noisy, None
            if self.demodulate:                                   # denoise_frame's demodulation
                x, var, how = demodulated(g, noisy, var)
            if live is not None:                                  # the pixels that were not traced, from their traced neighbours
                x, var = upsample(x, g, live, var=var, stream=st, **lattice)
            nxt = 1 if self._cur == 0 else 0
            out, out_var, length, *flags = accumulate(x, var, g, self._cam, self.history, self._blocks[nxt], alpha=frame_alpha(ds, g.tri),
                                                      stream=st, **moving, **self.params)
            if self.denoise is not None:
                out, out_var = denoise(out, g.tri, g.normal, g.point, var=out_var, stream=st, **self.denoise)
            if how is not None:
                out, out_var = remodulated(g, out, out_var, how)
            rgb = tonemap(out) if self.film is None else self.film(out, stream=st)
        self._cur, self._cam, self.noisy, self.live = nxt, N.Camera.from_buffer_copy(bytes(cam)), noisy, live
        self.flags = flags[0] if flags else None
        self.frames += 1
        return out, out_var, length, rgb
