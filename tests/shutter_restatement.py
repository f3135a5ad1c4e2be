"""include/squigly_shutter.h's contract -- the instant of a sub-ray, the pose of an instant, the lens ray under that pose -- restated in
numpy float32 on top of lens_restatement.py.

The rotation matrix (sqo_rot_matrix_rads under TRIG_CRD) and the fifth generator word (tfgen_words(~base)[4]) come from the oracle;
a sub-ray under a pose is lens_restatement.sub_ray's, unchanged; every other operation is a single float32 operation written out
here.  tests/test_shutter.py pins this module to the oracle's camera and holds sq_shutter_pose to it; tests/test_gpu_shutter.py holds
the kernels to it.

A motion is (pos0, ang0, pos1, ang1), each three numbers; time_jitter is passed beside it."""
import ctypes as C
import functools

import numpy as np
import pyoracle as O

import lens_restatement as LR
import sky_restatement as SR

f32 = np.float32
W, H, S = LR.W, LR.H, LR.S
# the test motion: data/camera as the shutter opens; a step aside, forward and up, and a turn, as it closes
OPEN = ((0.0, 7.0, 0.75), (1.5707963267948966, 0.0, -0.09817477042468103))
CLOSE = ((1.0, 6.0, 1.25), (1.5707963267948966 + 0.25, 0.0, -0.09817477042468103 + 0.1))
MOTION = (OPEN[0], OPEN[1], CLOSE[0], CLOSE[1])
STILL = (OPEN[0], OPEN[1], OPEN[0], OPEN[1])
LENSES = dict(LR.LENSES, plain=LR.PLAIN)


def motion_f32(motion):
    return tuple(np.array(v, np.float64).astype(f32) for v in motion)


def pose(motion, tt):
    """(pos [3], rot [9]) at the instant tt: x0 + tt * (x1 - x0) per component, then rotMatrixRads of the three angles."""
    p0, a0, p1, a1 = motion_f32(motion)
    tt = f32(tt)
    with np.errstate(all="ignore"):
        pos = (p0 + (tt * (p1 - p0).astype(f32)).astype(f32)).astype(f32)
        ang = (a0 + (tt * (a1 - a0).astype(f32)).astype(f32)).astype(f32)
    rot = (C.c_float * 9)()
    O.lib().sqo_rot_matrix_rads(float(ang[0]), float(ang[1]), float(ang[2]), O.TRIG_CRD, rot)
    return pos, np.array(list(rot), f32)


def camera(motion, tt):
    """The pose at tt as the oracle's Camera."""
    pos, rot = pose(motion, tt)
    cam = O.Camera()
    cam.pos = O.V3(float(pos[0]), float(pos[1]), float(pos[2]))      # (ctypes takes a float32 through a double unchanged, NaN included)
    for i in range(9):
        cam.rot[i] = float(rot[i])
    return cam


def instant(time_jitter, S_, R, w, y, x, r):
    """tt of sub-ray r of pixel (y, x): (r + time_jitter * random01 m4) / R, m4 the fifth output of mkTFGen (NOT base)."""
    m4 = O.tfgen_words(~int(LR.seed_base(S_, R, w, y, x, r)))[4]
    with np.errstate(all="ignore"):
        return f32(f32(f32(r) + f32(f32(time_jitter) * LR.random01(m4))) / f32(R))


def sub_ray(motion, time_jitter, lens, S_, R, w, h, y, x, r):
    """(o, d, base, tt) of sub-ray r of pixel (y, x): lens_restatement's sub-ray under the pose of its instant."""
    tt = instant(time_jitter, S_, R, w, y, x, r)
    o, d, base, _ = LR.sub_ray(camera(motion, tt), lens, S_, R, w, h, y, x, r)
    return o, d, base, tt


def rays(motion, time_jitter, lens, S_, R, w, h, rows=None, r_range=None):
    """lens_restatement.rays under the motion: (origins [nb, P, 3], directions [nb, P, 3], seeds [nb, P]) in the dense slot order."""
    rows = range(w) if rows is None else rows
    r0, r1 = (0, R) if r_range is None else r_range
    px = [(y, x) for y in rows for x in range(h)]
    o = np.zeros((r1 - r0, len(px), 3), f32)
    d = np.zeros_like(o)
    s = np.zeros((r1 - r0, len(px)), np.int64)
    for r in range(r0, r1):
        for i, (y, x) in enumerate(px):
            o[r - r0, i], d[r - r0, i], s[r - r0, i], _ = sub_ray(motion, time_jitter, lens, S_, R, w, h, y, x, r)
    return o, d, s


def trails(ob, flat, motion, time_jitter, lens, S_, R, w, h, rows=None):
    """lens_restatement.trails under the motion: trails[r][pixel][k]."""
    o, d, s = rays(motion, time_jitter, lens, S_, R, w, h, rows)
    n = S_ // R
    return [[[SR.path(ob, flat, O.tfgen_words(int(s[r, i]) + k), o[r, i], d[r, i]) for k in range(n)] for i in range(o.shape[1])]
            for r in range(R)]


@functools.lru_cache(maxsize=None)
def room_rays(lens_name, R, time_jitter):
    """rays of the room's W x H frame at S samples under MOTION, made once."""
    return rays(MOTION, time_jitter, LENSES[lens_name], S, R, W, H)


@functools.lru_cache(maxsize=None)
def room_trails(lens_name, R, time_jitter, which="bright"):
    """trails of the room's W x H frame at S samples and R sub-rays under MOTION and LENSES[lens_name], walked once."""
    c, _ = LR.room(which)
    o, d, s = room_rays(lens_name, R, time_jitter)
    n = S // R
    return [[[SR.path(c.ob, c.flat, O.tfgen_words(int(s[r, i]) + k), o[r, i], d[r, i]) for k in range(n)] for i in range(o.shape[1])]
            for r in range(R)]


def first_hits_at(ob, motion, tt, w=W, h=H):
    """The first-hit triangle of every pixel's plain ray under the pose at tt; -1 = Nothing."""
    cam = camera(motion, tt)
    want = [O.make_ray(w, h, y, x, cam) for y in range(w) for x in range(h)]
    return LR.first_hits(ob, np.array([r[0] for r in want], f32), np.array([r[1] for r in want], f32))
