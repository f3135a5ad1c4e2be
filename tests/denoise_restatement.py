"""The denoiser's two formulas (include/squigly_denoise.h) restated in numpy float32, one operation per line in the header's order.

Belongs here: `variance` and `denoise`, the specification the device kernels are held to bit for bit (tests/test_gpu_denoise.py)
and whose quality on the project's own scene tests/test_denoise.py checks; and `synthetic`, the seeded inputs both use.  The images
are processed whole, one shifted copy per tap: numpy rounds every operation to float32 and contracts nothing."""
import numpy as np

f = np.float32
K = (f(0.375), f(0.25), f(0.0625))
G = (f(0.5), f(0.25))
DEFAULTS = {"passes": 5, "sigma_l": 4.0, "eps_l": 1e-3, "sigma_p": 0.05, "normal_squarings": 3}


def lum(c):
    return (f(0.25) * c[..., 0] + f(0.5) * c[..., 1]) + f(0.25) * c[..., 2]


def variance(sums, sums2, counts):
    """sq_denoise_variance_device: float32 [...] from sums, sums2 [..., 3] and counts [...]."""
    s, q, c = np.asarray(sums, f), np.asarray(sums2, f), np.asarray(counts, np.int32)
    with np.errstate(all="ignore"):
        n = c.astype(f)[..., None]
        m = s / n
        d = q / n - m * m
        var = np.where(d > 0, d / (n - f(1)), f(0))
        v = (f(0.0625) * var[..., 0] + f(0.25) * var[..., 1]) + f(0.0625) * var[..., 2]
        l = lum(m)
        v = np.where(c < 2, l * l, v)
        v = np.where(c < 1, f(0), v)
    return v.astype(f)


def shifted(a, oy, ox):
    """(b, inside): b[y, x] = a[y + oy, x + ox] where that pixel is inside the image (zeros elsewhere), inside the mask of those."""
    rows, cols = a.shape[:2]
    b = np.zeros_like(a)
    inside = np.zeros((rows, cols), bool)
    y0, y1 = max(0, -oy), min(rows, rows - oy)
    x0, x1 = max(0, -ox), min(cols, cols - ox)
    if y0 < y1 and x0 < x1:
        b[y0:y1, x0:x1] = a[y0 + oy:y1 + oy, x0 + ox:x1 + ox]
        inside[y0:y1, x0:x1] = True
    return b, inside


def one_pass(C, V, valid, nrm, pnt, s, sigma_l, eps_l, sigma_p, squarings):
    rows, cols = valid.shape
    sd = None
    if V is not None:
        gs = np.zeros((rows, cols), f)
        gw = np.zeros((rows, cols), f)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                Vq, inside = shifted(V, dy, dx)
                ok = inside & shifted(valid, dy, dx)[0]
                g = G[abs(dy)] * G[abs(dx)]
                gs = np.where(ok, gs + g * Vq, gs)
                gw = np.where(ok, gw + g, gw)
        gv = gs / gw
        sd = sigma_l * np.sqrt(gv) + eps_l
    lp = lum(C)
    sw = np.zeros((rows, cols), f)
    sc = np.zeros((rows, cols, 3), f)
    sv = np.zeros((rows, cols), f)
    for dy in (-2, -1, 0, 1, 2):
        for dx in (-2, -1, 0, 1, 2):
            ok = shifted(valid, dy * s, dx * s)
            ok = ok[1] & ok[0]
            nq = shifted(nrm, dy * s, dx * s)[0]
            Pq = shifted(pnt, dy * s, dx * s)[0]
            Cq = shifted(C, dy * s, dx * s)[0]
            kw = K[abs(dy)] * K[abs(dx)]
            dn = (nrm[..., 0] * nq[..., 0] + nrm[..., 1] * nq[..., 1]) + nrm[..., 2] * nq[..., 2]
            t = np.where(dn > 0, dn, f(0))
            for _ in range(squarings):
                t = t * t
            e = Pq - pnt
            pd = (nrm[..., 0] * e[..., 0] + nrm[..., 1] * e[..., 1]) + nrm[..., 2] * e[..., 2]
            a = pd / sigma_p
            wz = f(1) / (f(1) + a * a)
            if V is not None:
                b = (lum(Cq) - lp) / sd
                wl = f(1) / (f(1) + b * b)
                w = ((kw * t) * wz) * wl
            else:
                w = (kw * t) * wz
            sw = np.where(ok, sw + w, sw)
            sc = np.where(ok[..., None], sc + w[..., None] * Cq, sc)
            if V is not None:
                Vq = shifted(V, dy * s, dx * s)[0]
                sv = np.where(ok, sv + (w * w) * Vq, sv)
    take = valid & (sw > 0)
    C1 = np.where(take[..., None], sc / sw[..., None], C)
    V1 = None if V is None else np.where(take, sv / (sw * sw), V)
    return C1, V1


def denoise(color, tri, normal, point, var=None, passes=5, sigma_l=4.0, eps_l=1e-3, sigma_p=0.05, normal_squarings=3):
    """sq_denoise_device: (out, out_var) float32 host arrays, out_var None without var."""
    C = np.array(color, f)
    V = None if var is None else np.array(var, f)
    valid = np.asarray(tri) >= 0
    nrm, pnt = np.asarray(normal, f), np.asarray(point, f)
    with np.errstate(all="ignore"):
        for i in range(passes):
            C, V = one_pass(C, V, valid, nrm, pnt, 1 << i, f(sigma_l), f(eps_l), f(sigma_p), int(normal_squarings))
    return C, V


def synthetic(rows, cols, seed, background=0.3):
    """Seeded inputs (color, var, tri, normal, point) of a rows x cols image: unit normals drawn from a handful of planes plus
    noise, points on those planes, about `background` of the pixels invalid in blobs and single pixels, heavy-tailed colours,
    variances with exact zeros."""
    rng = np.random.default_rng(seed)
    n_planes = 4
    base = rng.normal(size=(n_planes, 3))
    base /= np.linalg.norm(base, axis=-1, keepdims=True)
    offs = rng.uniform(-1, 1, n_planes)
    yy, xx = np.mgrid[0:rows, 0:cols]
    which = ((yy // 7 + xx // 11) % n_planes + (rng.random((rows, cols)) < 0.05) * rng.integers(0, n_planes, (rows, cols))) % n_planes
    nrm = base[which] + 0.02 * rng.normal(size=(rows, cols, 3))
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    # a point of the pixel's plane: the plane's foot point plus in-plane offsets that follow the pixel grid
    u = np.cross(base, np.roll(base, 1, axis=0))
    u /= np.linalg.norm(u, axis=-1, keepdims=True)
    v = np.cross(base, u)
    pnt = (offs[which][..., None] * base[which] + (0.03 * xx)[..., None] * u[which] + (0.03 * yy)[..., None] * v[which]
           + 0.002 * rng.normal(size=(rows, cols, 3)))
    tri = rng.integers(0, 1000, (rows, cols)).astype(np.int32)
    blobs = np.zeros((rows, cols), bool)
    for _ in range(max(1, rows * cols // 100)):
        cy, cx, r = rng.integers(0, rows), rng.integers(0, cols), rng.uniform(1, 4) * min(1.0, rows * cols / 200)   # a small image keeps valid pixels
        blobs |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
    blobs |= rng.random((rows, cols)) < background / 3
    tri[blobs] = -1
    color = np.abs(rng.standard_cauchy((rows, cols, 3))) * (rng.random((rows, cols, 1)) < 0.7)
    var = rng.exponential(1.0, (rows, cols)) * (rng.random((rows, cols)) < 0.8)
    return color.astype(f), var.astype(f), tri, nrm.astype(f), pnt.astype(f)
