"""The denoiser's real test frame: data/scene.obj (the room) at 48 rows x 64 columns and 16 samples, from the CPU oracle.

Belongs here: the frame's per-sample radiances folded into the moments a masked call keeps, its guides (first-hit triangle, point
and unit normal per pixel) and the 1024-sample frame it is judged against -- computed once per session and handed out unchanged."""
import numpy as np

from f32_folds import fold
from masked_calls import oracle_samples
from render_options import THREADS

f32 = np.float32
W, H, SPP, REF_SPP = 48, 64, 16, 1024
_ROOM = {}


def room(O, oracle_scene):
    """dict: sums, sums2 [W, H, 3], counts [W, H], avg (the 16-sample mean), tri, point, normal (the guides), ref (1024 samples)."""
    if _ROOM:
        return _ROOM
    ob, cam, _ = oracle_scene
    samples = oracle_samples(ob, cam, SPP, W, H, key="denoise-room")
    sums, sums2 = fold(samples, 0, SPP)
    with np.errstate(all="ignore"):
        avg = (f32(1) / f32(SPP)) * sums
    flat = ob.flatten()
    tri = np.full((W, H), -1, np.int32)
    point = np.zeros((W, H, 3), f32)
    normal = np.zeros((W, H, 3), f32)
    for y in range(W):
        for x in range(H):
            hit = ob.intersect(*O.make_ray(W, H, y, x, cam))
            if hit.hit:
                t = flat[hit.tri]
                n = np.cross(t["b"] - t["a"], t["c"] - t["a"]).astype(f32)
                tri[y, x] = hit.tri
                point[y, x] = (hit.point.x, hit.point.y, hit.point.z)
                normal[y, x] = n / np.sqrt((n * n).sum(dtype=f32), dtype=f32)
    ref, _, _ = ob.render(cam, REF_SPP, W, H, threads=THREADS, want_rgb=False)
    _ROOM.update(sums=sums, sums2=sums2, counts=np.full((W, H), SPP, np.int32), avg=avg.astype(f32), tri=tri, point=point,
                 normal=normal, ref=ref)
    return _ROOM
