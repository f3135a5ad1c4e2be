"""The frame's arithmetic around a sample, restated in numpy float32: the left folds of src/Lib.hs:85-88, the average and the
tonemap of its result.

Belongs here: a fold, an average or a tonemap that takes radiances as given and rounds where the kernels round.  What computes a
radiance (a path, a light's term) is a restatement's (depth_restatement, sky_restatement, lights_restatement).  The functions differ
in what they fold over and where they round, which is why there are several: do not merge them."""
import numpy as np

f32 = np.float32


def from_zero(r):
    with np.errstate(all="ignore"):
        return (f32(0) + r).astype(f32)                               # a one-sample fold: 0 + r


def fold_list(rs):
    """foldl (+) 0 over a list of [n, 3] float32 radiances, in float32."""
    s = np.zeros_like(rs[0])
    with np.errstate(all="ignore"):
        for r in rs:
            s = (s + r).astype(f32)
    return s


def fold(samples, a, b, s=None, q=None):
    """The float32 left folds of r and of r * r (the product rounded before the add) over the samples [a, b), continued from s, q."""
    s = np.zeros(samples.shape[1:], f32) if s is None else s.copy()
    q = np.zeros(samples.shape[1:], f32) if q is None else q.copy()
    with np.errstate(all="ignore"):
        for k in range(a, b):
            r = samples[k]
            s = s + r
            q = q + r * r
    return s, q


def avg_by_counts(sums, counts):
    """(1 / count) *^ sum per pixel, a pixel without samples dividing by 1."""
    with np.errstate(all="ignore"):
        return (f32(1) / np.maximum(counts, 1).astype(f32))[..., None] * sums


def tonemaps(O, avg):
    """The oracle's tonemap of every [..., 3] average, as RGB8 of the same shape."""
    return np.array([O.tonemap(a) for a in avg.reshape(-1, 3)], np.uint8).reshape(avg.shape)


def tonemap_image(O, avg):
    """The oracle's tonemap of a [rows, h, 3] image, pixel by pixel from Python floats."""
    return np.array([[O.tonemap(tuple(float(v) for v in px)) for px in row] for row in avg], np.uint8)
