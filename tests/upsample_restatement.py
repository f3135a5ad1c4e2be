"""The sparse-frame contract (include/squigly_denoise.h: sq_denoise_sparse_mask_device, sq_denoise_upsample_device) restated in numpy
float32, one operation per line in the header's order.

Belongs here: `lattice`, `gather`, `sparse_mask`, `upsample` and `lattice_offset`, the specification the two kernels and the host
program tests/upsample_main.cpp are held to bit for bit; `replicate`, the nearest-lattice baseline the quality test compares with;
and `synthetic` / `handmade`, the seeded guides both use.  The images are processed whole, one gather per tap: numpy rounds every
operation to float32 and contracts nothing."""
import numpy as np

f = np.float32
DEFAULTS = {"sigma_p": 0.0353, "cos_n": 0.9}         # sigma_p: denoise.default_sigma_p of the room (data/scene.obj)


def lattice_offset(frame, s):
    j = frame % (s * s)
    return j % s, (j // s + j % s) % s


def lattice(rows, cols, s, oy, ox):
    """bool [rows, cols]: the pixels on the lattice."""
    yy, xx = np.mgrid[0:rows, 0:cols]
    return ((yy - oy) % s == 0) & ((xx - ox) % s == 0)


def gather(tri, normal, point, s, oy, ox, sigma_p, cos_n, color=None, var=None):
    """(sw, sc, sv) of every pixel as if none were on the lattice (the callers look at the others only); sc, sv None without color, var."""
    tri = np.asarray(tri, np.int32)
    nrm, pnt = np.asarray(normal, f), np.asarray(point, f)
    rows, cols = tri.shape
    sigma_p, cos_n, fs = f(sigma_p), f(cos_n), f(s)
    yy, xx = np.mgrid[0:rows, 0:cols]
    yl = (yy - oy) // s * s + oy                      # numpy's // is the floor division
    xl = (xx - ox) // s * s + ox
    hit = tri >= 0
    sw = np.zeros((rows, cols), f)
    sc = None if color is None else np.zeros((rows, cols, 3), f)
    sv = None if var is None else np.zeros((rows, cols), f)
    with np.errstate(all="ignore"):
        ty = (yy - yl).astype(f) / fs
        tx = (xx - xl).astype(f) / fs
        for j in (0, 1):
            for i in (0, 1):
                qy, qx = yl + j * s, xl + i * s
                inside = (qy >= 0) & (qy < rows) & (qx >= 0) & (qx < cols)
                gy, gx = np.clip(qy, 0, rows - 1), np.clip(qx, 0, cols - 1)
                q_hit = tri[gy, gx] >= 0
                nq, Pq = nrm[gy, gx], pnt[gy, gx]
                dn = (nrm[..., 0] * nq[..., 0] + nrm[..., 1] * nq[..., 1]) + nrm[..., 2] * nq[..., 2]
                d = Pq - pnt
                pd = (nrm[..., 0] * d[..., 0] + nrm[..., 1] * d[..., 1]) + nrm[..., 2] * d[..., 2]
                on_surface = q_hit & (dn >= cos_n) & (np.abs(pd) <= sigma_p)
                acc = inside & np.where(hit, on_surface, ~q_hit)
                bw = (tx if i else f(1) - tx) * (ty if j else f(1) - ty)
                sw = np.where(acc, sw + bw, sw)
                if sc is not None:
                    sc = np.where(acc[..., None], sc + bw[..., None] * np.asarray(color, f)[gy, gx], sc)
                if sv is not None:
                    sv = np.where(acc, sv + bw * np.asarray(var, f)[gy, gx], sv)
    return sw, sc, sv


def sparse_mask(tri, normal, point, s, oy, ox, sigma_p=DEFAULTS["sigma_p"], cos_n=DEFAULTS["cos_n"]):
    """sq_denoise_sparse_mask_device: uint8 [rows, cols]."""
    rows, cols = np.asarray(tri).shape
    sw, _, _ = gather(tri, normal, point, s, oy, ox, sigma_p, cos_n)
    return (lattice(rows, cols, s, oy, ox) | ~(sw > 0)).astype(np.uint8)


def upsample(color, tri, normal, point, mask, s, oy, ox, var=None, sigma_p=DEFAULTS["sigma_p"], cos_n=DEFAULTS["cos_n"]):
    """sq_denoise_upsample_device: (out, out_var); out_var None without var."""
    c = np.asarray(color, f)
    rows, cols = np.asarray(tri).shape
    sw, sc, sv = gather(tri, normal, point, s, oy, ox, sigma_p, cos_n, c, var)
    fill = (np.asarray(mask) == 0) & ~lattice(rows, cols, s, oy, ox) & (sw > 0)
    with np.errstate(all="ignore"):
        out = np.where(fill[..., None], sc / sw[..., None], c).astype(f)
        out_var = None if var is None else np.where(fill, sv / sw, np.asarray(var, f)).astype(f)
    return out, out_var


def sparse_frame(color, var, tri, normal, point, s, oy, ox, **stops):
    """(mask, out, out_var) of a dense frame seen through the sparse pipeline: the mask of its guides; every pixel the mask leaves
    out was not traced, so it is overwritten with NaN first; then the fill.  A NaN in `out` that `color` does not have at a lattice
    pixel or a hole is a pixel that was read without having been traced."""
    mask = sparse_mask(tri, normal, point, s, oy, ox, **stops)
    dead = mask == 0
    c = np.where(dead[..., None], f(np.nan), np.asarray(color, f))
    v = None if var is None else np.where(dead, f(np.nan), np.asarray(var, f))
    out, out_var = upsample(c, tri, normal, point, mask, s, oy, ox, var=v, **stops)
    return mask, out, out_var


def replicate(color, s, oy, ox):
    """Every pixel takes the colour of the lattice pixel at or before it (the first one inside the image where that lies outside):
    what a sparse frame shows without a reconstruction."""
    c = np.asarray(color, f)
    rows, cols = c.shape[:2]
    yy, xx = np.mgrid[0:rows, 0:cols]
    yl, xl = (yy - oy) // s * s + oy, (xx - ox) // s * s + ox
    yl, xl = np.where(yl < 0, yl + s, yl), np.where(xl < 0, xl + s, xl)
    return c[np.clip(yl, 0, rows - 1), np.clip(xl, 0, cols - 1)]


def synthetic(rows, cols, seed, odd=False):
    """Seeded inputs (color, var, tri, normal, point): a floor of two levels 0.3 apart (more than any sigma_p used) split along a
    wavy line, patches tilted by up to ~35 degrees against the floor's normal, a few back-facing ones, about 15 % misses in blobs
    and single pixels, and smooth noise on the points so that |pd| straddles sigma_p = 0.05.  odd: NaN, +-inf and -0 in every
    field, at seeded pixels."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:rows, 0:cols].astype(np.float64)
    level = np.where(xx + 3 * np.sin(yy / 3.0) > cols * 0.55, 0.3, 0.0)
    pnt = np.stack([xx * 0.1, yy * 0.1, level + 0.04 * rng.normal(size=(rows, cols))], -1)
    nrm = np.zeros((rows, cols, 3))
    nrm[..., 2] = 1.0
    tilt = rng.random((rows, cols)) < 0.25
    nrm[tilt] += rng.normal(size=(int(tilt.sum()), 3)) * 0.35
    back = rng.random((rows, cols)) < 0.05
    nrm[back] *= -1.0
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    tri = rng.integers(0, 1000, (rows, cols)).astype(np.int32)
    miss = rng.random((rows, cols)) < 0.06
    for _ in range(max(1, rows * cols // 300)):
        cy, cx, r = rng.integers(0, rows), rng.integers(0, cols), rng.uniform(1, 4)
        miss |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
    if rows * cols > 1:
        tri[miss] = -1
        nrm[miss] = 0
        pnt[miss] = 0
    color = np.abs(rng.standard_cauchy((rows, cols, 3)))
    var = rng.exponential(1.0, (rows, cols)) * (rng.random((rows, cols)) < 0.8)
    out = [color.astype(f), var.astype(f), tri, nrm.astype(f), pnt.astype(f)]
    if odd:
        specials = np.array([np.nan, np.inf, -np.inf, -0.0], f)
        for a in (out[0], out[1], out[3], out[4]):
            at = rng.random(a.shape) < 0.04
            a[at] = specials[rng.integers(0, 4, int(at.sum()))]
    return tuple(out)


def handmade():
    """A 7 x 9 frame by hand, with NaN, +-inf and -0 in every field: (color, var, tri, normal, point).  Row 0 and column 0 lie before
    the lattice at offset (1, 1); the left half is a plane z = 0, the right half z = 1 (an edge for every sigma_p < 1), one column of
    sky between them and one sky pixel alone."""
    rows, cols = 7, 9
    nan, inf = np.nan, np.inf
    tri = np.arange(rows * cols, dtype=np.int32).reshape(rows, cols)
    tri[:, 4] = -1
    tri[5, 7] = -1
    nrm = np.zeros((rows, cols, 3), f)
    nrm[..., 2] = 1
    pnt = np.zeros((rows, cols, 3), f)
    yy, xx = np.mgrid[0:rows, 0:cols]
    pnt[..., 0], pnt[..., 1], pnt[..., 2] = xx, yy, (xx > 4)
    color = (1 + yy[..., None] * 10 + xx[..., None] + np.arange(3) * 0.25).astype(f)
    var = (0.5 + 0.01 * yy * xx).astype(f)
    # guides: a NaN normal at a lattice pixel of offset (0, 0) and at a pixel between; infinite and -0 points; a back-facing normal
    nrm[2, 2] = (nan, 0, 1)
    nrm[3, 1] = (0, nan, 1)
    nrm[4, 6] = (0, 0, -1)
    nrm[0, 8] = (-0.0, -0.0, 1)
    nrm[6, 0] = (inf, 0, 1)
    nrm[5, 3] = (-inf, 0, 1)
    pnt[2, 6] = (inf, 2, 1)
    pnt[1, 7] = (7, -inf, 1)
    pnt[4, 2] = (2, 4, nan)
    pnt[0, 0] = (-0.0, -0.0, -0.0)
    pnt[6, 8] = (8, 6, -0.0)
    # colours and variances: at lattice pixels (they are taps) and between (they are never read, or copied through)
    color[0, 0] = (nan, 1, 2)
    color[2, 0] = (inf, -inf, -0.0)
    color[0, 2] = (-0.0, -0.0, -0.0)
    color[1, 1] = (nan, inf, -0.0)
    color[3, 3] = (-inf, 3, nan)
    color[4, 8] = (inf, inf, inf)
    color[2, 5] = (nan, nan, nan)
    var[0, 0], var[2, 2], var[1, 1], var[4, 8], var[3, 5], var[6, 6], var[0, 6] = nan, inf, -0.0, -inf, nan, -0.0, inf
    return color, var, tri, nrm, pnt
