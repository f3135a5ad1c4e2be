"""The display stage (include/squigly_film.h) restated in numpy, one float32 operation per line, and the value tables its tests share.

Belongs here: the contract's arithmetic -- luminance and slot, histogram, the exposure chain, the five curves, the table, the
quantiser -- with nothing of the library in it.  The arctangent is the oracle's (sqo_atanf, its binary64 series rounded once), and
curve 0's bytes are the oracle's tonemap (pyoracle.tonemap through f32_folds.tonemaps): neither is restated a second time."""
import ctypes as C

import numpy as np

import f32_folds

f32 = np.float32
SLOTS = 2048
CURVES = ("reference", "atan", "reinhard", "filmic", "linear")
METER = dict(key=0.18, permille=500, e_min=2.0 ** -10, e_max=2.0 ** 10, rate=1.0, fallback=1.0)
BAYER = np.array([[0, 32, 8, 40, 2, 34, 10, 42],
                  [48, 16, 56, 24, 50, 18, 58, 26],
                  [12, 44, 4, 36, 14, 46, 6, 38],
                  [60, 28, 52, 20, 62, 30, 54, 22],
                  [3, 35, 11, 43, 1, 33, 9, 41],
                  [51, 19, 59, 27, 49, 17, 57, 25],
                  [15, 47, 7, 39, 13, 45, 5, 37],
                  [63, 31, 55, 23, 61, 29, 53, 21]], np.int32)
PI_F = f32(3.14159265358979323846)


def quiet(fn):
    def wrapped(*a, **kw):
        with np.errstate(all="ignore"):
            return fn(*a, **kw)
    wrapped.__name__, wrapped.__doc__ = fn.__name__, fn.__doc__
    return wrapped


def atan(O, x):
    """The oracle's float32 arctangent of every element."""
    L = O.lib()
    L.sqo_atanf.restype, L.sqo_atanf.argtypes = C.c_float, [C.c_float, C.c_int]
    x = np.asarray(x, f32)
    return np.array([L.sqo_atanf(float(v), O.TRIG_CRD) for v in x.reshape(-1)], f32).reshape(x.shape)


@quiet
def luminance(c):
    a = f32(0.25) * c[..., 0]
    b = f32(0.5) * c[..., 1]
    ab = a + b
    d = f32(0.25) * c[..., 2]
    return (ab + d).astype(f32)


def slot(L):
    """The histogram slot of every luminance."""
    L = np.asarray(L, f32)
    with np.errstate(all="ignore"):
        s = (np.ascontiguousarray(L).view(np.uint32) >> 20).astype(np.int64)
        s = np.where(L == np.inf, SLOTS - 1, s)
        return np.where(L > 0, s, 0)


def histogram(color):
    return np.bincount(slot(luminance(np.asarray(color, f32).reshape(-1, 3))), minlength=SLOTS).astype(np.int64)


def usable(p):
    return p is not None and bool(np.isfinite(p)) and bool(p > 0)


@quiet
def expose(hist, prev=None, **meter):
    """The exposure, a float32, of a histogram (2048 counts) and the exposure before it (None = none)."""
    m = dict(METER, **meter)
    hist = [int(v) for v in hist]
    p = None if prev is None else f32(prev)
    M = sum(hist[1:SLOTS - 1])
    if M == 0:
        return p if usable(p) else f32(m["fallback"])
    rank = max(1, (M * int(m["permille"]) + 999) // 1000)
    run, s = 0, 1
    for s in range(1, SLOTS - 1):
        run += hist[s]
        if run >= rank:
            break
    Lp = np.array([(s << 20) | 0x80000], np.uint32).view(f32)[0]
    t = f32(m["key"]) / Lp
    if t < f32(m["e_min"]):
        t = f32(m["e_min"])
    if t > f32(m["e_max"]):
        t = f32(m["e_max"])
    if not usable(p):
        return f32(t)
    step = f32(t - p)
    move = f32(f32(m["rate"]) * step)
    return f32(p + move)


def hmax(x, y):
    return np.where(x <= y, y, x)          # Haskell's Ord default: a NaN on either side selects per the comparison


def hmin(x, y):
    return np.where(x <= y, x, y)


@quiet
def atan_scale(O, x):
    mx = hmax(hmax(x[..., 0], x[..., 1]), x[..., 2])
    mn = hmin(hmin(x[..., 0], x[..., 1]), x[..., 2])
    s = mx + mn
    lightness = f32(0.5) * s
    half_pi = PI_F / f32(2)
    intensity = atan(O, lightness) / half_pi
    return (intensity / mx).astype(f32)


@quiet
def filmic(v):
    a = f32(2.51) * v
    a = a + f32(0.03)
    num = v * a
    b = f32(2.43) * v
    b = b + f32(0.59)
    den = v * b
    den = den + f32(0.14)
    return (num / den).astype(f32)


@quiet
def table(lut, d):
    lut = np.asarray(lut, f32)
    n = len(lut)
    v = np.where(d > 0, d, f32(0)).astype(f32)
    v = np.where(v > 1, f32(1), v).astype(f32)
    t = v * f32(n - 1)
    i = np.minimum(t.astype(np.int64), n - 2)
    f = t - i.astype(f32)
    lo, hi = lut[i], lut[i + 1]
    rise = hi - lo
    fr = f * rise
    return (lo + fr).astype(f32)


@quiet
def quantise(d, th):
    q = d * f32(255.0)
    q = (q + th).astype(f32)
    inside = (q > 0) & (q < 255)
    b = np.where(inside, q, 0).astype(np.int64)
    return np.where(q >= 255, 255, np.where(q > 0, b, 0)).astype(np.uint8)


@quiet
def develop(O, color, exposure=1.0, curve="reference", white=np.inf, lut=None, dither=False):
    """(rgb uint8, display float32) of a [rows, cols, 3] float32 image."""
    color = np.asarray(color, f32)
    rows, cols = color.shape[:2]
    x = (f32(exposure) * color).astype(f32)
    if curve == "reference":
        assert lut is None and not dither
        return f32_folds.tonemaps(O, x), (atan_scale(O, x)[..., None] * x).astype(f32)
    if curve == "atan":
        d = atan_scale(O, x)[..., None] * x
    elif curve == "reinhard":
        L = luminance(x)
        w2 = f32(white) * f32(white)
        t = L / w2
        t = f32(1) + t
        Ld = L * t
        one = f32(1) + L
        Ld = Ld / one
        s = Ld / L
        d = s[..., None] * x
    elif curve == "filmic":
        d = filmic(x)
    else:
        assert curve == "linear"
        d = x
    d = d.astype(f32)
    if lut is not None:
        d = table(lut, d)
    if dither:
        yy, xx = np.indices((rows, cols))
        th = (BAYER[yy & 7, xx & 7].astype(f32) + f32(0.5)) * f32(0.015625)
        th = th.astype(f32)[..., None]
    else:
        th = f32(0.5)
    return quantise(d, th), d


def chain(O, frames, film, auto=None):
    """Film(**film, auto=auto) over a list of frames: [(rgb, exposure)] -- the state carried from frame to frame."""
    out, state = [], None
    for c in frames:
        e = f32(film.get("exposure", 1.0))
        if auto is not None:
            e = state = expose(histogram(c), state, **auto)
        out.append((develop(O, c, e, **{k: v for k, v in film.items() if k != "exposure"})[0], e))
    return out


# ---- value tables ----
def bits(words):
    return np.array(words, np.uint32).view(f32)


def edge_values():
    """Every edge the contract names, as float32: NaN, +-inf, -0, negatives, subnormals, values over 1, the slot boundaries 2^k and
    their neighbours, and what lands at the ends of a table."""
    nan, inf = np.nan, np.inf
    v = [0.0, -0.0, nan, inf, -inf, -1.0, -1e-3, 1e-45, 1e-40, 1.1754942e-38, 1.17549435e-38, 3.4028235e38, 1e30, 1e-30,
         0.25, 0.5, 0.999, 1.0, 1.0000001, 1.5, 2.0, 4.5, 7.0, 100.0, 255.0, 256.0, 1e4, 0.18, 0.0019, 0.00392, 0.00393, 0.996, 0.9981]
    for k in (-126, -20, -1, 0, 1, 7, 127):
        p = f32(2.0) ** f32(k)
        v += [np.nextafter(p, f32(0)), p, np.nextafter(p, f32(inf))]
    for s in (1, 7, 8, 9, 1015, 1016, 2039):                   # the first and last value of a slot
        v += list(bits([s << 20, ((s + 1) << 20) - 1]))
    return np.array(v, f32)


def value_table(n_pixels, seed):
    """n_pixels colours: the edge values in all three places of a pixel (alone, paired with ordinary values, and against each other),
    then seeded ordinary radiances over six decades, some of them grey (mx == mn) and some black (mx == 0)."""
    rng = np.random.default_rng(seed)
    e = edge_values()
    px = [[a, a, a] for a in e] + [[a, 0.5, 0.25] for a in e] + [[0.25, a, 2.0] for a in e] + [[0.5, 0.125, a] for a in e]
    px += [[e[i], e[(i * 7 + 3) % len(e)], e[(i * 11 + 5) % len(e)]] for i in range(len(e))]
    px += [[0.001, -1000.0, 0.001], [-3.0, -2.0, -1.0], [-0.5, 2.0, 0.25]]      # a negative component: values over 1 and below 0 after the curve
    px = np.array(px, f32)
    rnd = (10.0 ** rng.uniform(-4, 2, (max(n_pixels, 1), 3))).astype(f32)
    rnd[rng.random(len(rnd)) < 0.1] = 0
    grey = rng.random(len(rnd)) < 0.1
    rnd[grey] = rnd[grey][:, :1]
    allpx = np.concatenate([px, rnd])
    take = rng.permutation(len(allpx))[:n_pixels] if n_pixels < len(px) else np.arange(n_pixels)
    return np.ascontiguousarray(allpx[take])


def slot_image(rows, cols, seed):
    """An image whose luminances fall in every slot 0 .. 2039 and in 2047, with NaN and negative pixels: rows * cols >= 2100."""
    rng = np.random.default_rng(seed)
    n = rows * cols
    img = np.zeros((n, 3), f32)
    s = np.arange(0, 2040)
    L = bits((s.astype(np.uint64) << 20) + rng.integers(1 << 18, 3 << 18, len(s)).astype(np.uint64))       # the middle half of a slot
    with np.errstate(over="ignore"):
        img[:2040, 1] = L * f32(2)                              # green alone: 0.5 * (2 L) = L exactly
    img[2032:2040] = L[2032:2040, None]                         # the top stop, where 2 L overflows: grey, whose luminance is L to an ulp
    img[2040] = [np.inf, 0, 0]
    img[2041] = [np.nan, 1, 1]
    img[2042] = [-1, -2, -3]
    img[2043] = [np.inf, -np.inf, 0]                            # inf - inf: NaN
    img[2044] = [np.inf, np.inf, np.inf]
    img[2045:] = (10.0 ** rng.uniform(-3, 1, (n - 2045, 3))).astype(f32)
    return img.reshape(rows, cols, 3)
