"""ctypes binding of libsquigly_film.so (include/squigly_film.h) and the driver around it.

The library is the display stage of the device pipeline: it meters a frame's luminance (histogram), settles an exposure on the device
(expose) and develops the fp32 frame into an 8-bit image (develop) under one of five tone curves, an optional transfer table and an
optional ordered dither.  PyTorch is the plumbing (device memory, streams); every byte comes from the HIP kernels of csrc/sq_film.hip.
There is no fallback: a missing library raises.
"""
import ctypes as C
import math

import numpy as np

from . import _native as N
from . import _plumbing as P

# include/squigly_film.h
EXPORTED_SYMBOLS = ["sq_film_last_error", "sq_film_build_id", "sq_film_histogram_device", "sq_film_expose_device", "sq_film_develop_device"]

SLOTS = 2048
CURVES = {"reference": 0, "atan": 1, "reinhard": 2, "filmic": 3, "linear": 4}
METER_DEFAULTS = {"key": 0.18, "permille": 500, "e_min": 2.0 ** -10, "e_max": 2.0 ** 10, "rate": 1.0, "fallback": 1.0}


class Meter(C.Structure):
    """sq_film_meter."""
    _fields_ = [("key", C.c_float), ("permille", C.c_int32), ("e_min", C.c_float), ("e_max", C.c_float), ("rate", C.c_float),
                ("fallback", C.c_float)]


class Params(C.Structure):
    """sq_film_params."""
    _fields_ = [("exposure", C.c_float), ("curve", C.c_int32), ("white", C.c_float), ("n_lut", C.c_int32), ("dither", C.c_int32)]


def _declare(L):
    vp, i32 = C.c_void_p, C.c_int32
    L.sq_film_histogram_device.argtypes = [i32, i32, i32, vp, vp, vp]
    L.sq_film_expose_device.argtypes = [i32, vp, C.POINTER(Meter), vp, vp, vp]
    L.sq_film_develop_device.argtypes = [i32, i32, i32, vp, vp, C.POINTER(Params), vp, vp, vp, vp]


_B = N.Binding("libsquigly_film.so", "sq_film_", _declare)
LIB_PATH, lib, check, build_id = _B
load = _B.load           # load(path): a variant build with its argument types declared (tools/gpu_film.py loads one beside the product's)


def _number(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise N.SquiglyError(f"{name} must be a number, got {v!r}")
    return float(v)


def make_meter(**kw):
    """sq_film_meter from keyword arguments over METER_DEFAULTS; what the library would refuse is refused here, before any device work."""
    unknown = set(kw) - set(METER_DEFAULTS)
    if unknown:
        raise N.SquiglyError(f"unknown meter parameter(s) {sorted(unknown)}: expected any of {sorted(METER_DEFAULTS)}")
    m = dict(METER_DEFAULTS, **kw)
    if not P.is_integer(m["permille"]) or not 1 <= int(m["permille"]) <= 1000:
        raise N.SquiglyError(f"permille must be an integer in 1..1000, got {m['permille']!r}")
    f = {k: _number(k, m[k]) for k in ("key", "e_min", "e_max", "rate", "fallback")}
    if not (0 < f["e_min"] <= f["e_max"] < math.inf):
        raise N.SquiglyError(f"e_min and e_max must be finite with 0 < e_min <= e_max, got {m['e_min']!r}, {m['e_max']!r}")
    if not 0 <= f["rate"] <= 1:
        raise N.SquiglyError(f"rate must be a number in 0..1, got {m['rate']!r}")
    if not f["fallback"] > 0:
        raise N.SquiglyError(f"fallback must be a number > 0, got {m['fallback']!r}")
    return Meter(f["key"], int(m["permille"]), f["e_min"], f["e_max"], f["rate"], f["fallback"])


def curve_index(curve):
    if isinstance(curve, str) and curve in CURVES:
        return CURVES[curve]
    if P.is_integer(curve) and 0 <= int(curve) < len(CURVES):
        return int(curve)
    raise N.SquiglyError(f"curve must be one of {sorted(CURVES, key=CURVES.get)}, got {curve!r}")


def make_params(exposure=1.0, curve="reference", white=math.inf, n_lut=0, dither=False):
    """sq_film_params; what the library would refuse of them is refused here."""
    c = curve_index(curve)
    w = _number("white", white)
    if c == CURVES["reinhard"] and not w > 0:
        raise N.SquiglyError(f"white must be a number > 0, got {white!r}")
    if not isinstance(dither, (bool, np.bool_)):
        raise N.SquiglyError(f"dither must be True or False, got {dither!r}")
    if c == 0 and (n_lut or dither):
        raise N.SquiglyError("the reference curve takes neither a table nor dither: it is the renderer's own conversion to bytes")
    return Params(_number("exposure", exposure), c, w, int(n_lut), int(bool(dither)))


def srgb_lut(n=4096):
    """The sRGB transfer function at n evenly spaced points of 0..1, float32 (built in numpy: a table is an input of develop)."""
    return _lut(n, lambda v: np.where(v <= 0.0031308, 12.92 * v, 1.055 * np.power(v, 1 / 2.4) - 0.055))


def gamma_lut(g, n=4096):
    """v ** (1 / g) at n evenly spaced points of 0..1, float32."""
    g = _number("g", g)
    if not 0 < g < math.inf:
        raise N.SquiglyError(f"g must be a finite number > 0, got {g!r}")
    return _lut(n, lambda v: np.power(v, 1 / g))


def _lut(n, fn):
    if not P.is_integer(n) or not 2 <= int(n) <= 65536:
        raise N.SquiglyError(f"a table has 2..65536 entries, got {n!r}")
    return np.ascontiguousarray(fn(np.linspace(0.0, 1.0, int(n))), np.float32)


def _frame(color):
    """(rows, cols, device) of a colour image: leading dimensions are flattened into rows."""
    import torch
    if (not isinstance(color, torch.Tensor) or color.dim() < 2 or color.shape[-1] != 3 or color.dtype != torch.float32 or not color.is_cuda
            or not color.is_contiguous()):
        got = f"{color.dtype} {tuple(color.shape)} on {color.device}" if isinstance(color, torch.Tensor) else type(color).__name__
        raise N.SquiglyError(f"color must be a contiguous torch.float32 CUDA tensor of shape [..., cols, 3], got {got}")
    cols = int(color.shape[-2])
    rows = int(color.numel() // (3 * cols)) if cols else 0
    if rows < 1 or cols < 1:
        raise N.SquiglyError(f"rows and cols must be at least 1 (got {rows} x {cols})")
    if rows * cols > 2 ** 31 - 1:
        raise N.SquiglyError(f"{rows} x {cols} pixels exceed 2^31 - 1 pixels in one call")
    return rows, cols, color.device


def histogram(color, out=None, stream=None):
    """sq_film_histogram_device: the luminance histogram of `color` (float32 [..., cols, 3]) as an int32 tensor of SLOTS counts (the
    bits are the library's uint32; a frame has at most 2^31 - 1 pixels).  Enqueued on `stream`."""
    import torch
    rows, cols, dev = _frame(color)
    if out is not None:
        P.tensor("out", out, (SLOTS,), torch.int32, dev)
    _, st = P.call_stream(dev, stream)
    with torch.cuda.stream(st):
        if out is None:
            out = torch.empty((SLOTS,), dtype=torch.int32, device=dev)
        check(lib().sq_film_histogram_device(dev.index or 0, rows, cols, color.data_ptr(), out.data_ptr(), P.stream_ptr(st)))
    return out


def expose(hist, prev=None, out=None, stream=None, **meter):
    """sq_film_expose_device: the exposure (a float32 tensor of one element) from a histogram and, optionally, the exposure before it;
    out may be prev (a state updated in place).  meter: any of METER_DEFAULTS.  Enqueued on `stream`."""
    import torch
    m = make_meter(**meter)
    if not isinstance(hist, torch.Tensor) or not hist.is_cuda:
        raise N.SquiglyError("hist must be an int32 CUDA tensor of 2048 counts (histogram())")
    dev = hist.device
    P.tensor("hist", hist, (SLOTS,), torch.int32, dev)
    if prev is not None:
        P.tensor("prev", prev, (1,), torch.float32, dev)
    if out is not None:
        P.tensor("out", out, (1,), torch.float32, dev)
    _, st = P.call_stream(dev, stream)
    with torch.cuda.stream(st):
        if out is None:
            out = torch.empty((1,), dtype=torch.float32, device=dev)
        check(lib().sq_film_expose_device(dev.index or 0, hist.data_ptr(), C.byref(m), P.ptr(prev), out.data_ptr(), P.stream_ptr(st)))
    return out


def develop(color, exposure=1.0, curve="reference", white=math.inf, lut=None, dither=False, out=None, want_display=False, stream=None):
    """sq_film_develop_device on device tensors: the uint8 image of color's shape, or (image, display) with want_display -- display
    being the float32 values the bytes were quantised from.  exposure: a number, or a float32 CUDA tensor of one element (expose()).
    curve: a name of CURVES.  lut: a float32 CUDA tensor of 2..65536 entries, or None.  out: the uint8 tensor, or (uint8, float32
    display) tensors, to receive the result (None = allocate).  Enqueued on `stream`."""
    import torch
    rows, cols, dev = _frame(color)
    e_t = exposure if isinstance(exposure, torch.Tensor) else None
    if e_t is not None:
        P.tensor("exposure", e_t, (1,), torch.float32, dev)
    n_lut = 0
    if lut is not None:
        if not isinstance(lut, torch.Tensor) or lut.dim() != 1:
            raise N.SquiglyError("lut must be a float32 CUDA tensor of 2..65536 entries (torch.from_numpy(srgb_lut()).cuda())")
        n_lut = int(lut.shape[0])
        if not 2 <= n_lut <= 65536:
            raise N.SquiglyError(f"a table has 2..65536 entries, got {n_lut}")
        P.tensor("lut", lut, (n_lut,), torch.float32, dev)
    par = make_params(1.0 if e_t is not None else exposure, curve, white, n_lut, dither)
    outs = tuple(out) if isinstance(out, (tuple, list)) else (() if out is None else (out,))
    if len(outs) > 2 or (len(outs) == 2 and not want_display):
        raise N.SquiglyError("out must be the uint8 image, or (image, display) with want_display")
    rgb, disp = outs + (None,) * (2 - len(outs))
    if rgb is not None:
        P.tensor("out image", rgb, tuple(color.shape), torch.uint8, dev)
    if disp is not None:
        P.tensor("out display", disp, tuple(color.shape), torch.float32, dev)
    _, st = P.call_stream(dev, stream)
    with torch.cuda.stream(st):
        if rgb is None:
            rgb = torch.empty(tuple(color.shape), dtype=torch.uint8, device=dev)
        if want_display and disp is None:
            disp = torch.empty(tuple(color.shape), dtype=torch.float32, device=dev)
        check(lib().sq_film_develop_device(dev.index or 0, rows, cols, color.data_ptr(), P.ptr(e_t), C.byref(par), P.ptr(lut), rgb.data_ptr(),
                                           P.ptr(disp), P.stream_ptr(st)))
    return (rgb, disp) if want_display else rgb


class Glare:
    """The glare of a Film (denoise.glare's parameters): what of the exposed frame is brighter than `threshold` -- saturating at `ceiling` --
    is carried down `levels` pyramid levels and up again, each coarser level weighing `spread` in the one above it, and added to the
    frame at `strength`.  A value object: what the library would refuse is refused here."""
    __slots__ = ("threshold", "ceiling", "levels", "spread", "strength")

    def __init__(self, threshold=1.0, ceiling=16.0, levels=5, spread=0.5, strength=0.1):
        from .denoise import make_glare_params
        make_glare_params(threshold=threshold, ceiling=ceiling, levels=levels, spread=spread, strength=strength)
        for name, v in (("threshold", threshold), ("ceiling", ceiling), ("spread", spread), ("strength", strength)):
            object.__setattr__(self, name, float(v))
        object.__setattr__(self, "levels", int(levels))

    def __setattr__(self, name, value):
        raise AttributeError("a Glare does not change: make another")

    def params(self):
        return {name: getattr(self, name) for name in self.__slots__}

    def __eq__(self, other):
        return isinstance(other, Glare) and self.params() == other.params()

    def __hash__(self):
        return hash(tuple(self.params().values()))

    def __repr__(self):
        return "Glare(" + ", ".join(f"{k}={v!r}" for k, v in self.params().items()) + ")"


def balance_arg(balance):
    """balance= of a Film: None, or three numbers (the white balance's factors for r, g, b) as floats."""
    if balance is None:
        return None
    try:
        b = tuple(_number("balance", v) for v in balance)
    except TypeError:
        b = ()
    if len(b) != 3:
        raise N.SquiglyError(f"balance must be None or three numbers (r, g, b), got {balance!r}")
    return b


class Film:
    """The display stage as an object: film(avg) is the uint8 image of the float32 CUDA frame avg, developed on avg's device without a
    host wait.  curve, exposure, white, dither: develop's.  lut: a table as a numpy array or a tensor (srgb_lut(), gamma_lut(g)); it
    is uploaded once per device, by prepare(device) or else by the first film() call on that device -- a copy from host memory,
    the one thing here that may wait: a caller that must not wait on the host calls prepare(device) first.
    auto (None = the fixed `exposure`): a dict of meter parameters (METER_DEFAULTS); every call then runs histogram, expose over the
    film's own one-float state and develop under that exposure, so a sequence adapts at `rate` per frame.  exposure_state: that
    state (a Python float; None before the first frame; reading it waits for the device), settable for checkpoints; reset() forgets
    it.  The state lives on the device of the first frame: a frame from another device is refused until reset(), never exposed from
    nothing without a word.  Film() is the reference curve at exposure 1: the bytes the renderer itself writes.
    glare (a Glare) and balance (three white-balance factors), both None by default: with either, the frame is metered as before --
    unbloomed and unbalanced -- then denoise.glare makes the exposed, balanced frame with its glare (none without a Glare) in a
    tensor of its own, and develop takes that at exposure 1, which is exact."""

    def __init__(self, curve="reference", exposure=1.0, white=math.inf, lut=None, dither=False, auto=None, glare=None, balance=None):
        self.curve, self.exposure, self.white, self.dither = curve, exposure, white, dither
        if glare is not None and not isinstance(glare, Glare):
            raise N.SquiglyError(f"glare must be None or a Glare, got {glare!r}")
        self.glare, self.balance = glare, balance_arg(balance)
        if lut is not None and not hasattr(lut, "is_cuda"):
            lut = np.ascontiguousarray(lut, np.float32)
            if lut.ndim != 1 or not 2 <= lut.shape[0] <= 65536:
                raise N.SquiglyError(f"a table has 2..65536 entries, got shape {lut.shape}")
        self.lut = lut
        make_params(exposure, curve, white, 0 if lut is None else int(lut.shape[0]), dither)      # refused before any device work
        if auto is not None and not isinstance(auto, dict):
            raise N.SquiglyError(f"auto must be None or a dict of meter parameters, got {auto!r}")
        self.auto = None if auto is None else dict(auto)
        if self.auto is not None:
            make_meter(**self.auto)
        self._luts, self._state, self._pending = {}, None, None

    def prepare(self, device):
        """Uploads the table to `device` (an index or a torch.device) ahead of the first frame, so that no film() call copies from
        host memory; a film without a table has nothing to prepare.  Returns the film."""
        dev, _ = P.call_stream(device, None)
        self._lut_on(dev)
        return self

    def _lut_on(self, dev):
        import torch
        if self.lut is None:
            return None
        if dev not in self._luts:
            t = self.lut if isinstance(self.lut, torch.Tensor) else torch.from_numpy(self.lut)
            self._luts[dev] = t.to(device=dev, dtype=torch.float32).contiguous()
        return self._luts[dev]

    @property
    def exposure_state(self):
        if self._state is None:
            return self._pending
        v = float(self._state.cpu()[0])
        return v if 0 < v < math.inf else None

    @exposure_state.setter
    def exposure_state(self, value):
        value = None if value is None else _number("exposure_state", value)
        if self._state is None or value is None:
            self._state, self._pending = None, value
        else:
            self._state.fill_(value)

    def reset(self):
        """Forget the exposure of the frames before: the next frame is exposed at its own target."""
        self._state, self._pending = None, None

    def film(self, avg, stream=None):
        import torch
        _, _, dev = _frame(avg)
        _, st = P.call_stream(dev, stream)
        with torch.cuda.stream(st):
            lut = self._lut_on(dev)
            e = self.exposure
            if self.auto is not None:
                if self._state is not None and self._state.device != dev:
                    raise N.SquiglyError(f"this film's exposure state is on {self._state.device} and the frame on {dev}: reset() it, or use "
                                         "a film per device")
                if self._state is None:
                    # 0 is "no exposure before": expose takes a state that is not finite and > 0 as none
                    self._state = torch.full((1,), 0.0 if self._pending is None else self._pending, dtype=torch.float32, device=dev)
                    self._pending = None
                e = expose(histogram(avg, stream=st), prev=self._state, out=self._state, stream=st, **self.auto)
            if self.glare is not None or self.balance is not None:
                from .denoise import glare
                g = self.glare.params() if self.glare is not None else {"levels": 0}
                avg, e = glare(avg, exposure=e, gain=self.balance or (1.0, 1.0, 1.0), stream=st, **g), 1.0
            return develop(avg, exposure=e, curve=self.curve, white=self.white, lut=lut, dither=self.dither, stream=st)

    __call__ = film


def film_arg(film):
    """film= of render_adaptive, Temporal and render_sequence: None or a Film."""
    if film is not None and not isinstance(film, Film):
        raise ValueError(f"film must be None or a Film, got {film!r}")
    return film
