"""include/squigly_lens.h's contract -- jittered, thin-lens sub-rays and their ordered fold -- restated in numpy float32.

Threefish (tfgen_words), the crd sine and cosine, rotVert, makeRay, intersectBIH and the tonemap come from the oracle; a sub-ray's
samples are depth_restatement's walk (kept with its misses, as sky_restatement keeps them, so that one walk serves every depth and
sky); every other operation is a single float32 operation written out here.  tests/test_lens.py pins this module to the oracle
where the two meet (no jitter, no aperture), and tests/test_gpu_lens.py holds the kernels to it.

A lens is (jitter, aperture, focus); a sky is None or (up, down)."""
import functools
import os

import numpy as np
import pyoracle as O

import depth_restatement as DR
import sky_restatement as SR

f32 = np.float32
PLAIN = (0.0, 0.0, 1.0)          # no jitter, no aperture: makeRay's ray


def random01(n):
    return DR.random01(n)


def lens_words(base):
    """m0 .. m3: the first four outputs of mkTFGen (NOT base)."""
    return O.tfgen_words(~int(base))[:4]


def rot_vert(v, cam):
    r = O.lib().sqo_rot_vert(O.v3(v), cam.rot)
    return np.array([r.x, r.y, r.z], f32)


def seed_base(S, R, w, y, x, r):
    return S * (x + y * w) + r * (S // R)


def sub_ray(cam, lens, S, R, w, h, y, x, r):
    """(o, d, base, detail) of sub-ray r of pixel (y, x); detail = (xs, ys, lx, ly), lx = ly = None without an aperture."""
    L = O.lib()
    jitter, aperture, focus = (f32(v) for v in lens)
    base = seed_base(S, R, w, y, x, r)
    m = lens_words(base)
    pos, _ = O.camera_arrays(cam)
    with np.errstate(all="ignore"):
        ww, hh = f32(w), f32(h)
        xs = f32(f32(x) + f32(jitter * random01(m[0])))
        ys = f32(f32(y) + f32(jitter * random01(m[1])))
        xoffs = f32(f32(xs - f32(ww / f32(2))) / ww)
        yoffs = f32(f32(f32(hh / f32(2)) - ys) / hh)
        if aperture == 0:
            o, lx, ly = pos.copy(), None, None
            dloc = (f32(1), xoffs, yoffs)
        else:
            rad = f32(aperture * f32(np.sqrt(random01(m[2]))))
            th = f32(f32(f32(2) * f32(np.pi)) * random01(m[3]))
            lx = f32(rad * f32(L.sqo_cosf(th, O.TRIG_CRD)))
            ly = f32(rad * f32(L.sqo_sinf(th, O.TRIG_CRD)))
            o = (pos + rot_vert((f32(0), lx, ly), cam)).astype(f32)
            dloc = (f32(1), f32(xoffs - f32(lx / focus)), f32(yoffs - f32(ly / focus)))
        d = rot_vert(dloc, cam)
    return o, d, base, (xs, ys, lx, ly)


def rays(cam, lens, S, R, w, h, rows=None, r_range=None):
    """(origins [nb, P, 3], directions [nb, P, 3], seeds [nb, P]) of the sub-rays r_range (default: all) of the pixels of the global
    rows `rows` (default: all w), in the library's slot order."""
    rows = range(w) if rows is None else rows
    r0, r1 = (0, R) if r_range is None else r_range
    px = [(y, x) for y in rows for x in range(h)]
    o = np.zeros((r1 - r0, len(px), 3), f32)
    d = np.zeros_like(o)
    s = np.zeros((r1 - r0, len(px)), np.int64)
    for r in range(r0, r1):
        for i, (y, x) in enumerate(px):
            o[r - r0, i], d[r - r0, i], s[r - r0, i], _ = sub_ray(cam, lens, S, R, w, h, y, x, r)
    return o, d, s


def trails(ob, flat, cam, lens, S, R, w, h, rows=None):
    """trails[r][pixel][k]: the path (to the largest depth, misses kept) of sample k of sub-ray r of every pixel."""
    o, d, s = rays(cam, lens, S, R, w, h, rows)
    n = S // R
    return [[[SR.path(ob, flat, O.tfgen_words(int(s[r, i]) + k), o[r, i], d[r, i]) for k in range(n)] for i in range(o.shape[1])]
            for r in range(R)]


def sub_ray_sums(tr, depth, sky=None):
    """s_r [R, P, 3]: per sub-ray the left fold of its samples from +0, what sq_raytrace_rays_device leaves in d_sum."""
    out = np.zeros((len(tr), len(tr[0]), 3), f32)
    with np.errstate(all="ignore"):
        for r, per_pixel in enumerate(tr):
            for i, samples in enumerate(per_pixel):
                s = np.zeros(3, f32)
                for t in samples:
                    s = (s + SR.radiance(t, depth, sky)).astype(f32)
                out[r, i] = s
    return out


def fold(parts, S, r_range=None, start=None, start2=None):
    """(sum, sum2, avg) of the sub-ray sums parts[r] over r_range (default: all): sum = s_0, sum = sum + s_r; sum2 likewise of
    s_r * s_r; a range that starts above 0 carries on from start / start2.  avg = (1 / S) *^ sum."""
    r0, r1 = (0, len(parts)) if r_range is None else r_range
    with np.errstate(all="ignore"):
        if r0 == 0:
            s, q = parts[0].copy(), (parts[0] * parts[0]).astype(f32)
            first = 1
        else:
            s, q = np.array(start, f32), np.array(start2, f32)
            first = r0
        for r in range(first, r1):
            s = (s + parts[r]).astype(f32)
            q = (q + (parts[r] * parts[r]).astype(f32)).astype(f32)
        avg = ((f32(1) / f32(S)) * s).astype(f32)
    return s, q, avg


def tonemap(avg):
    flat = np.asarray(avg, f32).reshape(-1, 3)
    return np.array([O.tonemap(p) for p in flat], np.uint8).reshape(np.shape(avg))


def frame(tr, S, depth, sky=None):
    """(sum, sum2, avg, rgb), each [P, 3], of the whole frame whose walks are tr = trails(...)."""
    s, q, avg = fold(sub_ray_sums(tr, depth, sky), S)
    return s, q, avg, tonemap(avg)


# ---- the inputs the lens tests share -----------------------------------------------------------------------------------------------
W, H, S = 16, 24, 8                       # the frame of the GPU tests: 16 rows x 24 columns at 8 samples
LENSES = {"aa": (1.0, 0.0, 1.0), "dof": (0.0, 0.1, 3.0), "both": (0.5, 0.1, 3.0)}


def room(which="shipped"):
    """depth_restatement's case of data/scene.obj under the shipped materials (or the "bright" ones, under which most samples carry
    light), and the oracle's data/camera."""
    c = DR.case(which)
    return c, O.load_camera(os.path.join(DR.DATA, "camera"))


@functools.lru_cache(maxsize=None)
def room_trails(lens_name, R, which="bright"):
    """trails of the room's W x H frame at S samples and R sub-rays under LENSES[lens_name], walked once."""
    c, cam = room(which)
    return trails(c.ob, c.flat, cam, LENSES[lens_name], S, R, W, H)


def first_hits(ob, o, d):
    """The triangle intersectBIH gives each ray of o, d [..., 3]; -1 = Nothing."""
    flat_o, flat_d = o.reshape(-1, 3), d.reshape(-1, 3)
    out = np.full(len(flat_o), -1, np.int64)
    for i in range(len(flat_o)):
        hit = ob.intersect(flat_o[i], flat_d[i])
        if hit.hit:
            out[i] = hit.tri
    return out.reshape(o.shape[:-1])
