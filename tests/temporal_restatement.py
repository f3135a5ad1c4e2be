"""The temporal accumulation's contract (include/squigly_temporal.h) restated in numpy float32, one operation per line in the header's
order.

Belongs here: `project`, `accumulate` and `chain`, the specification the device kernel is held to bit for bit
(tests/test_gpu_temporal.py) and whose quality on the project's own scene tests/test_temporal.py checks; and `synthetic`, the seeded
two-plane frames both use.  The images are processed whole, one gather per tap: numpy rounds every operation to float32 and contracts
nothing.  A camera is (pos [3], rot [9] row-major), a history block a dict of plain images."""
import numpy as np

f = np.float32
# sigma_p is a length of the scene: 0.0353 is denoise.default_sigma_p of the room (data/scene.obj), what sqt.Temporal derives there
DEFAULTS = {"alpha_min": 0.1, "max_history": 32, "sigma_p": 0.0353, "cos_n": 0.9}
BLOCK_FIELDS = ("color", "var", "len", "tri", "normal", "point")


def camera(cam):
    """(pos, rot) float32 arrays of a camera given as a pair, or as anything with .pos and .rot (the library's and the oracle's)."""
    if hasattr(cam, "rot"):
        pos = cam.pos
        pos = [pos.x, pos.y, pos.z] if hasattr(pos, "x") else list(pos)
        return np.array(pos, f), np.array(list(cam.rot), f)
    return np.asarray(cam[0], f).reshape(3), np.asarray(cam[1], f).reshape(9)


def project(cam, rows, cols, point):
    """(ok, fx, fy) of the world points `point` [..., 3] in the rows x cols image of `cam`: fx the column, fy the row."""
    pos, rot = camera(cam)
    P = np.asarray(point, f)
    ww, hh = f(rows), f(cols)
    with np.errstate(all="ignore"):
        e = [P[..., c] - pos[c] for c in range(3)]
        k = [(e[0] * rot[3 * i] + e[1] * rot[3 * i + 1]) + e[2] * rot[3 * i + 2] for i in range(3)]
        front = k[0] > 0
        xo = k[1] / k[0]
        yo = k[2] / k[0]
        fx = xo * ww + ww / f(2)
        fy = hh / f(2) - yo * hh
        ok = front & (fx >= f(-1)) & (fx < hh) & (fy >= f(-1)) & (fy < ww)
    return ok, fx.astype(f), fy.astype(f)


def first_block(color, var, tri, normal, point):
    return accumulate(color, var, tri, normal, point, None, None)["block"]


def accumulate(color, var, tri, normal, point, prev_cam, prev, alpha=None, alpha_min=0.1, max_history=32, sigma_p=0.0353, cos_n=0.9):
    """sq_temporal_accumulate_device: dict(color, var, len, block); prev = the previous call's block or None."""
    c, v = np.array(color, f), np.array(var, f)
    tri = np.asarray(tri, np.int32)
    nrm, pnt = np.asarray(normal, f), np.asarray(point, f)
    rows, cols = tri.shape
    out_c, out_v, out_len = c.copy(), v.copy(), np.ones((rows, cols), np.int32)
    if prev is not None:
        alpha_min, sigma_p, cos_n = f(alpha_min), f(sigma_p), f(cos_n)
        with np.errstate(all="ignore"):
            ok, fx, fy = project(prev_cam, rows, cols, pnt)
            ok &= tri >= 0
            fx, fy = np.where(ok, fx, f(0)), np.where(ok, fy, f(0))       # (pixels without a projection take no tap: any finite value)
            x0, y0 = np.floor(fx), np.floor(fy)
            tx, ty = fx - x0, fy - y0
            ix, iy = x0.astype(np.int64), y0.astype(np.int64)
            sw = np.zeros((rows, cols), f)
            sc = np.zeros((rows, cols, 3), f)
            sv = np.zeros((rows, cols), f)
            m = np.full((rows, cols), 0x7fffffff, np.int64)
            for j in (0, 1):
                for i in (0, 1):
                    qy, qx = iy + j, ix + i
                    inside = ok & (qy >= 0) & (qy < rows) & (qx >= 0) & (qx < cols)
                    gy, gx = np.clip(qy, 0, rows - 1), np.clip(qx, 0, cols - 1)
                    acc = inside & (prev["tri"][gy, gx] >= 0)
                    nq, Pq, Cq, Vq, Lq = prev["normal"][gy, gx], prev["point"][gy, gx], prev["color"][gy, gx], prev["var"][gy, gx], prev["len"][gy, gx]
                    bw = (tx if i else f(1) - tx) * (ty if j else f(1) - ty)
                    dn = (nrm[..., 0] * nq[..., 0] + nrm[..., 1] * nq[..., 1]) + nrm[..., 2] * nq[..., 2]
                    acc &= dn >= cos_n
                    d = Pq - pnt
                    pd = (nrm[..., 0] * d[..., 0] + nrm[..., 1] * d[..., 1]) + nrm[..., 2] * d[..., 2]
                    acc &= np.abs(pd) <= sigma_p
                    sw = np.where(acc, sw + bw, sw)
                    sc = np.where(acc[..., None], sc + bw[..., None] * Cq, sc)
                    sv = np.where(acc, sv + bw * Vq, sv)
                    m = np.where(acc, np.minimum(m, Lq.astype(np.int64)), m)
            blend = sw > 0
            hc = sc / sw[..., None]
            hv = sv / sw
            m1 = np.where(blend, m + 1, 1)
            a = f(1) / m1.astype(f)
            a = np.where(a < alpha_min, alpha_min, a)
            if alpha is not None:
                al = np.asarray(alpha, f)
                a = np.where(a < al, al, a)
            bc = hc + a[..., None] * (c - hc)
            om = f(1) - a
            bv = (om * om) * hv + (a * a) * v
            out_c = np.where(blend[..., None], bc, c).astype(f)
            out_v = np.where(blend, bv, v).astype(f)
            out_len = np.where(blend, np.minimum(m1, int(max_history)), 1).astype(np.int32)
    block = dict(color=out_c, var=out_v, len=out_len, tri=tri.copy(), normal=nrm.copy(), point=pnt.copy())
    return dict(color=out_c, var=out_v, len=out_len, block=block)


def chain(frames, cams, alphas=None, **params):
    """The accumulation over frames: frames[f] = (color, var, tri, normal, point) rendered under cams[f]; alphas[f] or None.
    Returns the list of accumulate's results."""
    outs, prev, prev_cam = [], None, None
    for i, (frame, cam) in enumerate(zip(frames, cams)):
        r = accumulate(*frame, prev_cam, prev, alpha=None if alphas is None else alphas[i], **params)
        outs.append(r)
        prev, prev_cam = r["block"], cam
    return outs


IDENTITY = (1, 0, 0, 0, 1, 0, 0, 0, 1)
FAR_X, NEAR_X = 4.0, 2.0
FAR_TRI, NEAR_TRI = 10, 20


def turned(angle):
    """A rotation about z (row-major), for cameras that do not look straight down +x."""
    c, s = np.cos(angle), np.sin(angle)
    return (c, -s, 0, s, c, 0, 0, 0, 1)


def synthetic(rows, cols, seed, cam=((0, 0, 0), IDENTITY), noise=0.0, background=0.08):
    """Seeded inputs (color, var, tri, normal, point) of the rows x cols frame `cam` sees of two planes facing -x: a far wall at
    x = 4 (triangle 10) and in front of it a strip at x = 2 (-0.3 <= y <= 0.1; triangle 20).  A ray that meets neither (a camera that
    looks away) is background (tri -1, zeros), and so are about `background` of the pixels, in seeded blobs and single pixels.  The
    points lie on their plane exactly in x; noise > 0 perturbs normals and points (seeded), so that the two stops are not met
    trivially.  Colours are heavy-tailed with NaN and infinite ones, variances have exact zeros."""
    rng = np.random.default_rng(seed)
    pos, rot = camera(cam)
    pos, rot = pos.astype(np.float64), rot.astype(np.float64).reshape(3, 3)
    yy, xx = np.mgrid[0:rows, 0:cols].astype(np.float64)
    ww, hh = float(rows), float(cols)
    v = np.stack([np.ones_like(xx), (xx - ww / 2) / ww, (hh / 2 - yy) / hh], -1)      # makeRay, src/Lib.hs:107-114
    d = v @ rot                                                                        # rotVert: a row vector times the matrix
    tri = np.full((rows, cols), -1, np.int32)
    pnt = np.zeros((rows, cols, 3))
    with np.errstate(all="ignore"):
        for X, t_id, ylo, yhi in ((FAR_X, FAR_TRI, -np.inf, np.inf), (NEAR_X, NEAR_TRI, -0.3, 0.1)):    # far first: near wins
            t = (X - pos[0]) / d[..., 0]
            P = pos + t[..., None] * d
            hit = (t > 0) & (d[..., 0] > 0) & (P[..., 1] >= ylo) & (P[..., 1] <= yhi)
            P[..., 0] = X
            tri[hit] = t_id
            pnt[hit] = P[hit]
    if background:
        blobs = rng.random((rows, cols)) < background / 2
        for _ in range(max(1, rows * cols // 400)):
            cy, cx, r = rng.integers(0, rows), rng.integers(0, cols), rng.uniform(1, 3)
            blobs |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
        tri[blobs] = -1
        pnt[blobs] = 0
    nrm = np.zeros((rows, cols, 3))
    nrm[tri >= 0] = (-1.0, 0.0, 0.0)
    if noise:
        nrm += noise * rng.normal(size=nrm.shape) * (tri >= 0)[..., None]
        nrm[tri >= 0] /= np.linalg.norm(nrm[tri >= 0], axis=-1, keepdims=True)
        pnt += noise * rng.normal(size=pnt.shape) * (tri >= 0)[..., None]
    color = np.abs(rng.standard_cauchy((rows, cols, 3))) * (rng.random((rows, cols, 1)) < 0.8)
    odd = rng.random((rows, cols))
    color[odd < 0.03] = np.nan
    color[(odd >= 0.03) & (odd < 0.06), 1] = np.inf
    var = rng.exponential(1.0, (rows, cols)) * (rng.random((rows, cols)) < 0.8)
    return color.astype(f), var.astype(f), tri, nrm.astype(f), pnt.astype(f)
