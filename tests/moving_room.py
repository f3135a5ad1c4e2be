"""The moving-geometry test sequence: the room (data/scene.obj) plus a small diffuse box of its own material that hovers 0.1
above the floor and slides along x, seen by a still camera at 48 rows x 64 columns, eight frames of 16 samples from the CPU oracle.

Belongs here: the box (twelve triangles; frame f's vertices are the rest pose plus f * STEP rounded once, which is also what
sqt.moved_mesh gives), every frame's oracle scene, samples, guides and object table in that frame's tree order, the product's mesh and
poses of the same sequence, and the 1024-sample frames of the first and the last geometry -- computed once per session and handed out
unchanged.

The camera is data/camera's tipped straight down (its third angle taken to -pi / 2), under the ceiling at z = 1.9 above the box's
track: what it sees of the box is the top face, which the lamp in the ceiling lights directly.  That is what a judgement against a
1024-sample reference needs.  Under data/camera itself -- outside the open front of the room -- every face of a box that the
camera sees looks away from the lamp and is lit through paths of three rays alone: of the 560 samples a 16-sample frame spends on
such a face, 0 to 2 are not black (measured on a box at (x, 1.2, 0.2)), the reference's own pixels scatter between 0 and three times
their mean, and an error measured there compares where single samples happened to fall.  The top face is 3.2 below the camera, so
a step of 0.3 shifts its image by 48 * 0.3 / 3.2 = 4.5 columns a frame (the column offset is scaled by the row count).  The track
(y = -1.55) runs clear of the prism and the mirror."""
import numpy as np

import temporal_room as TR
from f32_folds import fold
from render_options import THREADS

f32 = np.float32
W, H, SPP, FRAMES, REF_SPP, PERIOD = TR.W, TR.H, TR.SPP, TR.FRAMES, TR.REF_SPP, TR.PERIOD
CAMERA_TEXT = b"-0.4 -1.55 1.9\n1.5707963267948966 0 -1.5707963267948966\n"
STEP = 0.3                                    # along x, a frame
BOX_CENTRE, BOX_HALF = (-1.05, -1.55, -1.6), 0.3
BOX_SURF = (0.7, 0.35, 0.15)
_SEQ = {}

_CORNERS = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float64)
_FACES = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]      # outward, counter-clockwise


def box_rest():
    """[12, 3, 3] float32: the box's triangles in the rest pose (frame 0)."""
    v = (np.array(BOX_CENTRE) + BOX_HALF * _CORNERS).astype(f32)
    return np.array([[v[a], v[b], v[c]] for q in _FACES for a, b, c in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))], f32)


def box_at(f):
    """Frame f's box: the rest pose plus f * STEP along x, in float64, rounded once."""
    return (box_rest().astype(np.float64) + np.array([f * STEP, 0.0, 0.0])).astype(f32)


def oracle_tris(O, room_tris, f):
    box = np.zeros(12, O.TRI_DTYPE)
    v = box_at(f)
    box["a"], box["b"], box["c"] = v[:, 0], v[:, 1], v[:, 2]
    box["surf"] = BOX_SURF
    return np.concatenate([room_tris, box])


def product_mesh(sqt, room_mesh):
    """(mesh, poses, box material): the room's mesh plus the box in its rest pose under a material of its own (the last), and the
    [FRAMES, n_materials, 3, 4] poses of the sequence: identity for the room's materials, the slide for the box's."""
    tris, mats = np.array(room_mesh.tris), np.array(room_mesh.materials)
    box = np.zeros(12, tris.dtype)
    v = box_rest()
    box["v0"], box["v1"], box["v2"], box["mat"] = v[:, 0], v[:, 1], v[:, 2], len(mats)
    mat = np.zeros(1, mats.dtype)
    mat["surf"] = BOX_SURF
    poses = np.tile(np.eye(3, 4), (FRAMES, len(mats) + 1, 1, 1))
    poses[:, len(mats), 0, 3] = STEP * np.arange(FRAMES)
    return sqt.Mesh.from_arrays(np.concatenate([tris, box]), np.concatenate([mats, mat])), poses, len(mats)


BACK = np.array([[1, 0, 0, -STEP, 0, 1, 0, 0, 0, 0, 1, 0]], f32)          # the box's move from a frame to the one before


def sequence(O, oracle_scene):
    """dict: cam, frames = per frame dict(sums, sums2, avg, guides, objects), ref (1024 samples of the last geometry), ref_first
    (of the first).  objects is the frame's table in its own tree's triangle order: 0 for the box, -1 for the room."""
    if _SEQ:
        return _SEQ
    room_tris = oracle_scene[2]
    cam = O.camera_from_text(CAMERA_TEXT)
    frames, obs = [], []
    for i in range(FRAMES):
        ob = O.BIH(oracle_tris(O, room_tris, i))
        obs.append(ob)
        k0 = (i % PERIOD) * SPP
        s = np.array([[[ob.sample_radiance(cam, SPP * PERIOD, W, H, y, x, k) for x in range(H)] for y in range(W)]
                      for k in range(k0, k0 + SPP)], f32)
        sums, sums2 = fold(s, 0, SPP)
        with np.errstate(all="ignore"):
            avg = (sums / f32(SPP)).astype(f32)
        flat = ob.flatten()
        objects = np.where((flat["surf"] == np.array(BOX_SURF, f32)).all(-1), 0, -1).astype(np.int32)
        assert (objects == 0).sum() == 12
        frames.append(dict(sums=sums, sums2=sums2, avg=avg, guides=TR.guides(O, ob, cam), objects=objects))
    ref, _, _ = obs[-1].render(cam, REF_SPP, W, H, threads=THREADS, want_rgb=False)
    ref_first, _, _ = obs[0].render(cam, REF_SPP, W, H, threads=THREADS, want_rgb=False)
    _SEQ.update(cam=cam, frames=frames, ref=ref, ref_first=ref_first)
    return _SEQ
