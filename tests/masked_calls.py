"""The masked range call (DeviceScene.render_rows_masked) as the adaptive and slot-fate tests drive it, and the oracle's samples
they fold.

Belongs here: the sentinel-filled output buffers of a masked call, the call itself brought to the host, and the per-sample radiances
of a frame from the CPU oracle (kept per key, computed once)."""
import numpy as np

from render_options import THREADS

f32 = np.float32
SENT = {"sums": 7.25, "sums2": 5.5, "avg": -3.5, "rgb": 123, "counts": 77}
_SAMPLES = {}


def oracle_samples(ob, cam_o, n, w, h, k_hi=None, cast=False, key=None):
    """[k_hi, w, h, 3] float32: the radiance of sample k of pixel (y, x) of the n-sample frame (a cast frame: its cast colour)."""
    k_hi = n if k_hi is None else k_hi
    ck = (key, n, w, h, k_hi, cast)
    if key is not None and ck in _SAMPLES:
        return _SAMPLES[ck]
    if cast:   # the cast colour of a pixel is the oracle's 1-sample cast frame (1 / 1 * c == c)
        c, _, _ = ob.render(cam_o, 1, w, h, cast=True, threads=THREADS)
        s = np.broadcast_to(c, (k_hi,) + c.shape).copy()
    else:
        s = np.array([[[ob.sample_radiance(cam_o, n, w, h, y, x, k) for x in range(h)] for y in range(w)] for k in range(k_hi)], f32)
    if key is not None:
        _SAMPLES[ck] = s
    return s


def buffers(rows, h):
    """The five output buffers of a masked call, filled with sentinels."""
    import torch
    mk = lambda shape, dt, v: torch.full(shape, v, dtype=dt, device="cuda:0")  # noqa: E731
    return {"sums": mk((rows, h, 3), torch.float32, SENT["sums"]), "sums2": mk((rows, h, 3), torch.float32, SENT["sums2"]),
            "counts": mk((rows, h), torch.int32, SENT["counts"]), "avg": mk((rows, h, 3), torch.float32, SENT["avg"]),
            "rgb": mk((rows, h, 3), torch.uint8, SENT["rgb"])}


def masked(ds, cam, n, w, h, a, b, B, mask, with_counts=True, with_sums2=True, **kw):
    import torch
    m = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask, np.uint8)).cuda()
    ds.render_rows_masked(cam, n, w, h, a, b, B["sums"], mask=m, sums2=B["sums2"] if with_sums2 else None,
                          counts=B["counts"] if with_counts else None, out_avg=B["avg"], out_rgb=B["rgb"], **kw)
    torch.cuda.synchronize()


def host(B):
    return {k: v.cpu().numpy() for k, v in B.items()}
