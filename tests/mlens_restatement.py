"""include/squigly_mlens.h's contract -- the live rule, the ascending list, the fold into the listed pixels with the pixel's own
divisor -- restated in numpy float32 on top of lens_restatement.py, and an adaptive driver over its sub-ray sums.

Belongs here: what the masked lens tests compare the library with, and the walks they share.  tests/test_mlens.py holds the driver's
populations on the CPU; tests/test_gpu_mlens.py holds the kernels and AdaptiveLens to this module."""
import functools

import numpy as np

import lens_restatement as LR

f32 = np.float32
W, H = LR.W, LR.H
P = W * H
# the adaptive cases: name -> (lens, S, R, eps); first = step = 2 sub-rays, tol = 0.5, depth 3, the "bright" room at W x H
TOL, FIRST, STEP = 0.5, 2, 2
CASES = {"a": ("aa", 8, 8, 1e-3), "b": ("both", 16, 8, 1e-3)}


def live(mask, counts, r_begin, pixels=None):
    """LIVE of every pixel as a bool array: mask and counts are flat arrays or None."""
    n = len(mask) if mask is not None else len(counts) if counts is not None else pixels
    out = np.ones(n, bool)
    if mask is not None:
        out &= np.asarray(mask).reshape(-1) != 0
    if r_begin != 0 and counts is not None:
        out &= np.asarray(counts).reshape(-1) == r_begin
    return out


def live_list(mask, counts, r_begin, pixels=None):
    """The live pixels in ascending order, int32."""
    return np.flatnonzero(live(mask, counts, r_begin, pixels)).astype(np.int32)


def indexed_fold(parts, index, n, r_begin, r_end, state):
    """sq_mlens_fold_device on host arrays.  parts [nb, L, 3]: the sub-ray sums s_(r_begin + i) of the listed pixels in list order;
    state: a dict of flat per-pixel arrays "sum" [P, 3] and any of "sum2", "count", "avg", "rgb", updated in place for the listed
    pixels (an entry outside [0, P) is skipped); n = S / R."""
    parts = np.asarray(parts, f32)
    index = np.asarray(index, np.int64)
    pixels = len(state["sum"])
    ok = (index >= 0) & (index < pixels)
    p = index[ok]
    with np.errstate(all="ignore"):
        if r_begin == 0:
            s = parts[0][ok].copy()
            q = (s * s).astype(f32)
            first = 1
        else:
            s = state["sum"][p].copy()
            q = state["sum2"][p].copy() if "sum2" in state else np.zeros_like(s)
            first = 0
        for b in range(first, parts.shape[0]):
            t = parts[b][ok]
            s = (s + t).astype(f32)
            q = (q + (t * t).astype(f32)).astype(f32)
        avg = ((f32(1) / f32(r_end * n)) * s).astype(f32)
    state["sum"][p] = s
    if "sum2" in state:
        state["sum2"][p] = q
    if "count" in state:
        state["count"][p] = r_end
    if "avg" in state:
        state["avg"][p] = avg
    if "rgb" in state:
        state["rgb"][p] = LR.tonemap(avg) if len(p) else np.zeros((0, 3), np.uint8)
    return state


@functools.lru_cache(maxsize=None)
def walk(lens_name, S, R, which="bright"):
    """The trails of the room's W x H frame (lens_restatement.trails), walked once per (lens, S, R); S = 8 shares
    lens_restatement.room_trails' walks."""
    if S == LR.S:
        return LR.room_trails(lens_name, R, which)
    c, cam = LR.room(which)
    return LR.trails(c.ob, c.flat, cam, LR.LENSES[lens_name], S, R, W, H)


@functools.lru_cache(maxsize=None)
def sub_ray_sums(lens_name, S, R, depth=3, sky=None):
    """s_r [R, P, 3] of the room's frame."""
    return LR.sub_ray_sums(walk(lens_name, S, R), depth, sky)


def adaptive(parts, n, rule, first=FIRST, step=STEP, mask=None, stop_after=None):
    """The loop of AdaptiveLens over the sub-ray sums parts [R, P, 3]: list, fold, rule, until no pixel is live or all R sub-rays
    are folded (or stop_after steps were taken).  rule(sums, sums2, counts, mask) -> mask, e.g. the product's rule_reference with
    eps * n * n.  Returns the state dict ("sum", "sum2", "count", "avg", "rgb", "mask", "done", "steps")."""
    R, pixels = parts.shape[0], parts.shape[1]
    st = {"sum": np.zeros((pixels, 3), f32), "sum2": np.zeros((pixels, 3), f32), "count": np.zeros(pixels, np.int32),
          "avg": np.zeros((pixels, 3), f32), "rgb": np.zeros((pixels, 3), np.uint8)}
    m = np.ones(pixels, np.uint8) if mask is None else np.asarray(mask, np.uint8).reshape(-1).copy()
    done, steps = 0, 0
    while done < R and (stop_after is None or steps < stop_after):
        index = live_list(m, st["count"], done)
        if len(index) == 0:
            break
        r_end = min(done + (first if done == 0 else step), R)
        indexed_fold(parts[done:r_end][:, index], index, n, done, r_end, st)
        done = r_end
        m = (np.asarray(rule(st["sum"], st["sum2"], st["count"], m)).reshape(-1) != 0).astype(np.uint8)
        steps += 1
    st.update(mask=m, done=done, steps=steps)
    return st


def stop_classes(counts, R, first=FIRST, step=STEP):
    """How many pixels stopped after each possible number of sub-rays, as a list over first, first + step, ..., R."""
    ends = list(range(first, R, step)) + [R]
    return [int((np.asarray(counts).reshape(-1) == e).sum()) for e in ends]
