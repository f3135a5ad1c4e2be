"""The temporal accumulation's real test sequence: data/scene.obj (the room) at 48 rows x 64 columns, eight frames of 16 samples under
a camera that steps sideways, from the CPU oracle.

Belongs here: the cameras, every frame's samples folded into the moments a masked call keeps, its guides and materials (first-hit
triangle, point, unit normal, surf, emit, reflective), the demodulation of denoise_frame restated in numpy, and the 1024-sample frame
of the last camera the sequence is judged against -- computed once per session and handed out unchanged."""
import numpy as np

from f32_folds import fold
from render_options import THREADS

f32 = np.float32
W, H, SPP, FRAMES, REF_SPP = 48, 64, 16, 8, 1024
PERIOD = 8                                  # frame f takes the samples [16 f, 16 f + 16) of the 128-sample frame
# data/camera is "0 7 0.75" looking down -y: the camera steps along x, 0.04 a frame
CAMERA_TEXTS = [b"%.2f 7 0.75\n1.5707963267948966 0 -0.09817477042468103\n" % (-0.14 + 0.04 * i) for i in range(FRAMES)]
_SEQ = {}


def guides(O, ob, cam):
    """dict: tri [W, H], point, normal, surf, emit [W, H, 3], reflective [W, H] of the first hits under cam (zeros where none)."""
    flat = ob.flatten()
    g = dict(tri=np.full((W, H), -1, np.int32), point=np.zeros((W, H, 3), f32), normal=np.zeros((W, H, 3), f32),
             surf=np.zeros((W, H, 3), f32), emit=np.zeros((W, H, 3), f32), reflective=np.zeros((W, H), f32))
    for y in range(W):
        for x in range(H):
            hit = ob.intersect(*O.make_ray(W, H, y, x, cam))
            if hit.hit:
                t = flat[hit.tri]
                n = np.cross(t["b"] - t["a"], t["c"] - t["a"]).astype(f32)
                g["tri"][y, x] = hit.tri
                g["point"][y, x] = (hit.point.x, hit.point.y, hit.point.z)
                g["normal"][y, x] = n / np.sqrt((n * n).sum(dtype=f32), dtype=f32)
                g["surf"][y, x], g["emit"][y, x], g["reflective"][y, x] = t["surf"], t["emissive"] * t["emit"], t["reflective"]
    return g


def demodulate(avg, var, g):
    """denoise_frame's demodulation in float32: (x, var', ok, scale)."""
    with np.errstate(all="ignore"):
        ok = (g["tri"] >= 0) & (g["surf"] > 0).all(-1)
        x = np.where(ok[..., None], (avg - g["emit"]) / np.where(ok[..., None], g["surf"], f32(1)), avg).astype(f32)
        ls = (f32(0.25) * g["surf"][..., 0] + f32(0.5) * g["surf"][..., 1]) + f32(0.25) * g["surf"][..., 2]
        scale = np.where(ok, ls * ls, f32(1)).astype(f32)
        return x, (var / scale).astype(f32), ok, scale


def remodulate(out, out_var, g, ok, scale):
    with np.errstate(all="ignore"):
        return np.where(ok[..., None], out * g["surf"] + g["emit"], out).astype(f32), (out_var * scale).astype(f32)


def sequence(O, oracle_scene):
    """dict: cams (the oracle's), frames = per frame dict(sums, sums2, avg, guides), ref (1024 samples under the last camera)."""
    if _SEQ:
        return _SEQ
    ob = oracle_scene[0]
    cams = [O.camera_from_text(t) for t in CAMERA_TEXTS]
    frames = []
    for i, cam in enumerate(cams):
        k0 = (i % PERIOD) * SPP
        s = np.array([[[ob.sample_radiance(cam, SPP * PERIOD, W, H, y, x, k) for x in range(H)] for y in range(W)]
                      for k in range(k0, k0 + SPP)], f32)       # the slice [k0, k0 + SPP) of masked_calls.oracle_samples(ob, cam, 128, W, H)
        sums, sums2 = fold(s, 0, SPP)
        with np.errstate(all="ignore"):
            avg = (sums / f32(SPP)).astype(f32)
        frames.append(dict(sums=sums, sums2=sums2, avg=avg, guides=guides(O, ob, cam)))
    ref, _, _ = ob.render(cams[-1], REF_SPP, W, H, threads=THREADS, want_rgb=False)
    _SEQ.update(cams=cams, frames=frames, ref=ref)
    return _SEQ
