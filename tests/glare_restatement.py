"""The glare stage (include/squigly_denoise.h: sq_denoise_glare_device) restated in numpy, one float32 operation per line, and the frames
its tests share.

Belongs here: the contract's arithmetic -- level sizes and workspace bytes, the exposed pixel, the bright pass, the down and up steps with
their clamped taps, the pyramid and the composite -- with nothing of the library in it; and the chain Film(glare=, balance=) stands
for, over tests/film_restatement.py's meter and curves."""
import numpy as np

import film_restatement as FR

f32 = np.float32
MAX_LEVELS = 8
MAX_PIXELS = 2 ** 31 - 1
DEFAULTS = dict(threshold=1.0, ceiling=16.0, levels=5, spread=0.5, strength=0.1)
A, B = f32(0.125), f32(0.375)
quiet = FR.quiet


def level_sizes(rows, cols, levels):
    """[(r_k, c_k)] for k < levels."""
    out = []
    for _ in range(levels):
        rows, cols = (rows + 1) // 2, (cols + 1) // 2
        out.append((rows, cols))
    return out


def work_bytes(rows, cols, levels):
    if rows < 1 or cols < 1 or rows * cols > MAX_PIXELS or not 0 <= levels <= MAX_LEVELS:
        return 0
    return 16 * sum(r * c for r, c in level_sizes(rows, cols, levels))


@quiet
def exposed(color, e, gain):
    x = f32(e) * np.asarray(color, f32)
    return (x * np.asarray(gain, f32)).astype(f32)


@quiet
def bright(x, threshold, ceiling):
    t, c = f32(threshold), f32(ceiling)
    L = FR.luminance(x)
    m = np.where(L < c, L, c).astype(f32)
    d = m - t
    s = np.where(L > t, d / L, f32(0)).astype(f32)
    b = (s[..., None] * x).astype(f32)
    b = np.where(b >= 0, b, f32(0)).astype(f32)            # a NaN compares false; -0 >= 0 holds, so a -0 stays
    return np.where(b > c, c, b).astype(f32)


def down_taps(n):
    """[4, (n + 1) // 2] fine coordinates: tap k of output o is 2o - 1 + k, clamped to the fine extent n."""
    o = np.arange((n + 1) // 2)
    return np.stack([np.clip(2 * o - 1 + k, 0, n - 1) for k in range(4)])


@quiet
def tap4(p0, p1, p2, p3):
    lo = A * p0 + B * p1
    hi = B * p2 + A * p3
    return (lo + hi).astype(f32)


def down(p):
    """D of a [r, c, 3] image: [(r + 1) // 2, (c + 1) // 2, 3]."""
    p = np.asarray(p, f32)
    tx, ty = down_taps(p.shape[1]), down_taps(p.shape[0])
    h = tap4(p[:, tx[0]], p[:, tx[1]], p[:, tx[2]], p[:, tx[3]])
    return tap4(h[ty[0]], h[ty[1]], h[ty[2]], h[ty[3]])


def up_taps(n, N):
    """(i0, i1, a, b) of the fine coordinates 0 .. n - 1 over a coarse extent N."""
    v = np.arange(n)
    i0 = (v - 1) >> 1
    a = np.where(v & 1, f32(0.75), f32(0.25)).astype(f32)
    return np.clip(i0, 0, N - 1), np.clip(i0 + 1, 0, N - 1), a, (f32(1) - a).astype(f32)


@quiet
def up(p, r, c):
    """U of a coarse [R, C, 3] image at the fine size r x c."""
    p = np.asarray(p, f32)
    y0, y1, ay, by = up_taps(r, p.shape[0])
    x0, x1, ax, bx = up_taps(c, p.shape[1])
    ax, bx = ax[None, :, None], bx[None, :, None]
    ay, by = ay[:, None, None], by[:, None, None]
    top = ax * p[y0][:, x0] + bx * p[y0][:, x1]
    bottom = ax * p[y1][:, x0] + bx * p[y1][:, x1]
    return (ay * top.astype(f32) + by * bottom.astype(f32)).astype(f32)


@quiet
def pyramid(x, threshold, ceiling, levels):
    """[B_0 .. B_levels-1] of an exposed frame x."""
    out, p = [], bright(x, threshold, ceiling)
    for _ in range(levels):
        p = down(p)
        out.append(p)
    return out


@quiet
def glare(color, exposure=1.0, gain=(1.0, 1.0, 1.0), threshold=1.0, ceiling=16.0, levels=5, spread=0.5, strength=0.1):
    """out of sq_denoise_glare_device for a [rows, cols, 3] float32 frame."""
    x = exposed(color, exposure, gain)
    if levels == 0:
        return x
    Bs = pyramid(x, threshold, ceiling, levels)
    a = Bs[-1]
    for k in range(levels - 2, -1, -1):
        u = f32(spread) * up(a, *Bs[k].shape[:2])
        a = (Bs[k] + u.astype(f32)).astype(f32)
    u = f32(strength) * up(a, *x.shape[:2])
    return (x + u.astype(f32)).astype(f32)


def chain(O, frames, film, auto=None, glare_params=None, balance=None):
    """Film(**film, auto=auto, glare=Glare(**glare_params), balance=balance) over a list of frames: [(rgb, exposure)].  The frame is
    metered as it is; glare() makes the exposed, balanced frame, and the curve takes that at exposure 1."""
    out, state = [], None
    for c in frames:
        e = f32(film.get("exposure", 1.0))
        if auto is not None:
            e = state = FR.expose(FR.histogram(c), state, **auto)
        g = dict(glare_params) if glare_params is not None else dict(levels=0)
        x = glare(c, e, balance or (1.0, 1.0, 1.0), **g)
        out.append((FR.develop(O, x, 1.0, **{k: v for k, v in film.items() if k != "exposure"})[0], e))
    return out


# ---- frames ----
def bright_edge_values(threshold, ceiling):
    """film_restatement's edge values and, with them, the values at and around the threshold and the ceiling."""
    t, c = f32(threshold), f32(ceiling)
    inf = f32(np.inf)
    around = [np.nextafter(t, -inf), t, np.nextafter(t, inf), np.nextafter(c, -inf), c, np.nextafter(c, inf), f32(2) * c, f32(0.5) * (t + c)]
    return np.concatenate([FR.edge_values(), np.array(around, f32)])


def bright_table(threshold, ceiling):
    """Every edge value in every channel position: alone in all three, beside ordinary values in each one, and against each other."""
    e = bright_edge_values(threshold, ceiling)
    px = [[a, a, a] for a in e] + [[a, 0.5, 0.25] for a in e] + [[0.25, a, 2.0] for a in e] + [[0.5, 0.125, a] for a in e]
    px += [[a, 3.0, 5.0] for a in e] + [[7.0, a, 2.0] for a in e] + [[20.0, 30.0, a] for a in e]          # glaring neighbours
    px += [[e[i], e[(i * 7 + 3) % len(e)], e[(i * 11 + 5) % len(e)]] for i in range(len(e))]
    return np.array(px, f32)


def value_frame(rows, cols, seed):
    """film_restatement's value table as a frame, scaled so that a good share of it glares under the default threshold, with NaN, inf,
    negative and 1e30 pixels planted wherever the frame is large enough to hold them."""
    px = FR.value_table(rows * cols, seed).reshape(rows, cols, 3).copy()
    rng = np.random.default_rng(seed + 1000)
    hot = rng.random((rows, cols)) < 0.2
    with np.errstate(all="ignore"):
        px[hot] = (px[hot] * f32(8)).astype(f32)
    return px


def random_frame(rows, cols, seed):
    """Radiances over four decades around 1 with NaN, +-inf, negative and 1e30 pixels planted."""
    rng = np.random.default_rng(seed)
    px = (10.0 ** rng.uniform(-2, 2, (rows, cols, 3))).astype(f32)
    plant = [[np.nan, 1, 1], [1, np.nan, np.nan], [np.inf, 1, 1], [-np.inf, 2, 2], [np.inf, np.inf, np.inf], [-1, -2, -3], [1e30, 1e30, 1e30],
             [-5, 20, 1], [3.4028235e38, 3.4028235e38, 3.4028235e38], [-0.0, 0.0, -0.0]]
    n = rows * cols
    if n >= 4 * len(plant):
        at = rng.permutation(n)[:len(plant)]
        px.reshape(-1, 3)[at] = np.array(plant, f32)
    return px
