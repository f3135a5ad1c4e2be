"""Randomised parity campaign for level-1 culling (sq_gen_bounce1, level1_culled; the packer's build_level1, level1_cover and
level1_mirror): random scenes with mirrors, random cameras inside them and small frames, through every call that runs sq_gen_bounce1,
with option "level1_cull" at 1 and at 0.  Each frame is held to the C oracle bit for bit, and sq_get_stats slots 28, 29 and 30 -- the
rays conditions (1)-(3), condition (4) alone and condition (5) alone drop -- to the counts the three restatements predict
(tests/level1_restatement.py, tests/level1_stretch_restatement.py, tests/level1_mirror_restatement.py).  A kernel that culls too little
still gives the oracle's frame; only the counts see it.  Expected values never come from the library's own counters.

    python tests/fuzz_level1.py [seconds=240] [first_seed=0]

prints one line per mismatch with the seed that reproduces it, and a summary.  tests/test_fuzz_level1.py judges the pytest slice
without a GPU (the lemma's counter-example search on every scene, and what the slice covers); tests/test_gpu_fuzz_level1.py runs it.

`case(seed)` draws everything from default_rng(seed), in this order (recorded seeds keep reproducing only while it stays):
  1. the family: one float.  Seeds with seed % 4 == 3 are edge scenes, EDGES[(seed // 4) % len(EDGES)] -- taken from the seed, so that
     every 68 consecutive seeds hold each of them once; the others are "room" (< 0.6), "soup" (< 0.8) or "lattice" by the float.
  2. the scene, by its family's function below, each in the order it is written; it ends with the scale and the rotation.
  3. the two cameras: the first inside the geometry (u < 0.8), one of fuzz_gpu.make_camera (u < 0.9), or far outside and looking
     away (a frame without a first-bounce ray); the second always inside.
  4. the frame: w, h in 4 .. 16 (the larger sides more often), spp in 1 .. 3.
  5. the live mask of the masked calls: a chequerboard or random.
  6. the options: overlap, slots, pool, resident, primary_resident, rng_table_mb, guided, cull.
"""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)
import pyoracle as O  # noqa: E402

import fuzz_gpu as F  # noqa: E402
import level1_mirror_restatement as M5  # noqa: E402
import level1_restatement as R  # noqa: E402
import level1_stretch_restatement as S  # noqa: E402
from bitcmp import canon, same  # noqa: E402
from render_options import DEFAULT_SLOTS, THREADS  # noqa: E402
from scenes import oracle_tris_of  # noqa: E402

sqt = importlib.import_module("squigly-trace_amd")      # importing the package loads no library: F.load_libraries does, when a case runs
f32 = np.float32
CULLED, STRETCH, MIRROR = 28, 29, 30                    # sq_get_stats slots
SIDES = np.arange(4, 17)
SIDE_WEIGHTS = np.where(SIDES >= 10, 3.0, 1.0) / np.where(SIDES >= 10, 3.0, 1.0).sum()
ROOM_SCALES = (0.05, 0.25, 1.0)
# The packer's bound on a triangle is P = 1.25 |e1| |e2| <= 29 (sq_cull_lemma.h, kLemmaPmax).  A wall triangle of room(2.0) has legs 4 and
# 4 sqrt 2: P = 28.284 at scale 1, 28.990 at 1.0124 and 29.019 at 1.0129 -- a part in a thousand either side, far above float32 rounding
P_UNDER, P_OVER = 1.0124, 1.0129
EDGES = ("P_under", "P_over", "emit63", "emit64", "emit65", "groups12", "groups13", "w8", "w9", "five_values", "refl_2", "refl_neg",
         "refl_nan", "sliver", "all_mirror", "no_mirror", "room_outside")


class Case:
    """One seed: scene, two cameras, frame, mask, options."""


# ---- scenes: each returns (v [n, 3, 3] float64 before scale and rotation, mats, mat, scales to choose from) ----------------------
def materials(rng, reflective, lamp_scatters=False):
    """One material per value of `reflective`, each with a surface colour in 0.2 .. 0.9, and the lamp's behind them: emissive, absorbing
    unless lamp_scatters."""
    n = len(reflective)
    mats = np.zeros(n + 1, sqt._native.MAT_DTYPE)
    mats["reflective"][:n] = reflective
    mats["surf"][:n] = rng.uniform(0.2, 0.9, (n, 3))
    mats["emissive"][n] = float(rng.choice([1.0, 15.0, 25.0]))
    mats["emit"][n] = rng.uniform(0.3, 1.0, 3)
    if lamp_scatters:
        mats["surf"][n] = rng.uniform(0.2, 0.9, 3)
    return mats


def lamp_quad(rng):
    """A small two-triangle lamp in the room [-2, 2]^3: free-standing, coplanar with a wall, or standing on one with an edge in it."""
    s = rng.uniform(0.2, 0.8, 2)
    how = int(rng.integers(0, 3))
    ax, sg = int(rng.integers(0, 3)), float(rng.choice([-1.0, 1.0]))
    a, b = [i for i in range(3) if i != ax]
    o = rng.uniform(-1.2, 1.0, 3)
    ex, ey = np.zeros(3), np.zeros(3)
    if how == 0:
        ex = rng.normal(0, 1, 3); ex *= s[0] / np.linalg.norm(ex)
        ey = np.cross(ex, rng.normal(0, 1, 3)); ey *= s[1] / np.linalg.norm(ey)
    elif how == 1:
        o[ax] = 2.0 * sg
        ex[a], ey[b] = s[0], s[1]
    else:
        o[ax] = 2.0 * sg
        ex[a], ey[ax] = s[0], -sg * s[1]
    return M5.quad(o, ex, ey).astype(np.float64)


def room_scene(rng, edge=None):
    """The closed cube of fuzz_gpu.room(2.0): six walls of 1 .. 4 distinct `reflective` values, 0 .. 40 clutter triangles, diffuse or
    mixed, 1 .. 3 lamp quads; `edge` bends one of these (EDGES)."""
    values = [0.0, 0.25, 0.5, 0.75, 1.0]
    n_vals = int(rng.integers(1, 5))
    vals = list(rng.choice(values, n_vals, replace=False))
    if edge == "five_values":
        vals = [0.2, 0.4, 0.6, 0.8, 1.0]
    elif edge == "all_mirror":
        vals = [1.0]
    elif edge == "no_mirror":
        vals = [0.0]
    n_vals = len(vals)
    wall_mat = rng.integers(0, n_vals, 6)
    wall_mat[:min(n_vals, 6)] = np.arange(min(n_vals, 6))                # every value on a wall
    wall_mat = wall_mat[rng.permutation(6)]
    n_clutter = int(rng.integers(0, 41))
    if edge in ("emit63", "emit64", "emit65"):
        n_clutter = int(edge[4:]) + int(rng.integers(8, 30))
    clutter = rng.uniform(-1.5, 1.5, (n_clutter, 1, 3)) + rng.normal(0, 0.3, (n_clutter, 3, 3))
    mixed = bool(rng.integers(0, 2)) or edge == "all_mirror"
    reflective = vals + [0.0]                                            # the diffuse clutter's material behind the walls'
    extra = {"refl_2": 2.0, "refl_neg": -1.0, "refl_nan": np.nan, "sliver": 1.0}.get(edge)
    if extra is not None:
        reflective = reflective + [extra]
    mats = materials(rng, reflective, lamp_scatters=rng.random() < 0.2)
    lamp = len(reflective)
    clutter_mat = rng.integers(0, n_vals, n_clutter) if mixed else np.full(n_clutter, n_vals)
    n_lamps = int(rng.integers(1, 4))
    lamps = [lamp_quad(rng) for _ in range(n_lamps)]
    wall_tri_mat = np.repeat(wall_mat, 2)
    if edge in ("emit63", "emit64", "emit65"):                           # that many clutter triangles are the lamps, and no quad
        clutter_mat[rng.choice(n_clutter, int(edge[4:]), replace=False)] = lamp
        lamps = []
    if edge in ("refl_2", "refl_neg", "refl_nan"):                       # one whole wall, non-emissive
        wall_tri_mat[2 * int(rng.integers(0, 6)):][:2] = lamp - 1
    v = [np.array(F.room(2.0)), clutter] + lamps
    mat = [wall_tri_mat, clutter_mat] + [np.full(2, lamp)] * len(lamps)
    if edge == "sliver":                                                 # a mirror 3 long and a few 1e-4 wide
        a, d = rng.uniform(-1.5, -0.5, 3), rng.normal(0, 1, 3)
        d /= np.linalg.norm(d)
        v.append(np.array([[a, a + 1.5 * d, a + 3.0 * d + rng.normal(0, 3e-4, 3)]]))
        mat.append(np.array([lamp - 1]))
    scales = (1.0 * P_UNDER,) if edge == "P_under" else (1.0 * P_OVER,) if edge == "P_over" else ROOM_SCALES
    return np.concatenate(v), mats, np.concatenate(mat), scales


def random_quads(rng, n):
    """n mirror quads for level1_mirror_restatement.mirror_soup: axis-aligned or tilted, sides 1.5 .. 3, values index 1 or 2."""
    out = []
    for _ in range(n):
        o = rng.uniform(-2.5, 0.5, 3)
        if rng.random() < 0.5:
            ax = int(rng.integers(0, 3))
            a, b = [i for i in range(3) if i != ax]
            ex, ey = np.zeros(3), np.zeros(3)
            ex[a], ey[b] = rng.uniform(1.5, 3, 2)
        else:
            ex = rng.normal(0, 1, 3); ex *= rng.uniform(1.5, 3) / np.linalg.norm(ex)
            ey = np.cross(ex, rng.normal(0, 1, 3)); ey *= rng.uniform(1.5, 3) / np.linalg.norm(ey)
        out.append((M5.quad(o, ex, ey), int(rng.integers(1, 3))))
    return out


def soup_scene(rng, edge=None):
    """level1_mirror_restatement.mirror_soup (a diffuse soup of level1_restatement.soup with planar mirrors and a clustered emitter
    group) with random quads and cluster point, or for three in ten level1_restatement.soup with a random mirror zone; the edges: n parallel mirror quads (12 fit the record, 13 do not) and one quad under
    8 or 9 emitters in general position (8 W vectors fit)."""
    sseed = int(rng.integers(0, 1 << 31))
    cluster = tuple(rng.uniform(-1.2, 1.2, 3))
    size = float(rng.uniform(0.4, 0.8))
    if edge in ("groups12", "groups13"):
        n = int(edge[6:])
        q = [(M5.quad((-1.5, -1.5, -2.0 + 0.3 * k), (3, 0, 0), (0, 3, 0)), 1 + k % 2) for k in range(n)]
        tris, mats, _ = M5.mirror_soup(sseed, 1, q, cluster=(1.2, 1.2, 2.6), emitter_size=0.5)
    elif edge in ("w8", "w9"):
        tris, mats, _ = M5.mirror_soup(sseed, int(edge[1:]), [(M5.quad((-1.5, -1.5, -2.5), (3, 0, 0), (0, 3, 0)), 2)])
    elif rng.random() < 0.3:                                             # level1_restatement.soup itself: mirrors of six values in one zone
        zone = tuple(rng.uniform(-1.2, 1.2, 3))
        tris, mats, _ = R.soup(sseed, int(rng.choice([1, 2, 12])), zoned=zone, cluster=cluster, emitter_size=size)
    else:
        n_emit = int(rng.choice([1, 2, 3, 6]))
        values =(0.0, 0.3, 0.7) if rng.random() < 0.5 else (0.0, float(rng.choice([0.25, 0.5, 1.0])), 1.0)
        tris, mats, _ = M5.mirror_soup(sseed, n_emit, random_quads(rng, int(rng.integers(1, 5))), values=values, cluster=cluster, emitter_size=size)
    v = np.stack([tris["v0"], tris["v1"], tris["v2"]], 1).astype(np.float64)
    return v, mats, tris["mat"].astype(np.int64), (1.0, 1.0, 0.25)


def lattice_scene(rng, edge=None):
    """fuzz_gpu.lattice -- unit right triangles on the faces of a grid: exact ties, coplanar panels, more planes than a record holds --
    with diffuse, half-mirror and mirror materials and 1 .. 4 lamp triangles."""
    v = F.lattice(rng, int(rng.integers(2, 5)))
    mats = materials(rng, [0.0, 0.5, 1.0])
    mat = rng.choice(3, len(v), p=[0.6, 0.2, 0.2])
    if rng.random() < 0.5:                                               # mirrors on the planes of one orientation only: fewer groups
        nrm = np.abs(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])).argmax(1)
        mat[nrm != int(rng.integers(0, 3))] = 0
    mat[rng.choice(len(v), min(len(v), int(rng.choice([1, 2, 4]))), replace=False)] = 3
    return v, mats, mat, (1.0, 0.25)


def camera_text(pos, ang):
    return (" ".join(F._fixed(p) for p in pos) + "\n" + " ".join(F._fixed(a) for a in ang) + "\n").encode()


def inside_camera(rng, reach):
    return camera_text(rng.uniform(-reach, reach, 3), rng.uniform(-3.2, 3.2, 3))


def away_camera(rng, far):
    """From far outside, the one of eight poses whose central ray points least at the scene."""
    pos = rng.normal(0, 1, 3)
    pos *= far / np.linalg.norm(pos)
    best = None
    for _ in range(8):
        text = camera_text(pos, rng.uniform(-3.2, 3.2, 3))
        _, d = O.make_ray(8, 8, 4, 4, O.camera_from_text(text))
        score = float(np.dot(d, -pos) / (np.linalg.norm(d) * far))
        if best is None or score < best[0]:
            best = (score, text)
    return best[1]


def case(seed):
    c = Case()
    c.seed = seed
    rng = np.random.default_rng(seed)
    # 1. the family
    u = rng.random()
    c.edge = EDGES[(seed // 4) % len(EDGES)] if seed % 4 == 3 else None
    if c.edge is not None:
        c.family = "soup" if c.edge in ("groups12", "groups13", "w8", "w9") else "room"
    else:
        c.family = "room" if u < 0.6 else "soup" if u < 0.8 else "lattice"
    # 2. the scene
    v, c.mats, c.mat, scales = {"room": room_scene, "soup": soup_scene, "lattice": lattice_scene}[c.family](rng, c.edge)
    c.scale = float(rng.choice(scales))
    c.rotated = bool(rng.integers(0, 2)) and c.family != "soup"          # (the soups' tilted quads are their rotations)
    q, _ = np.linalg.qr(rng.normal(0, 1, (3, 3)))                        # a random orthogonal matrix, drawn for every seed
    if c.rotated:
        v = v @ q.T
    c.v = (v * c.scale).astype(f32)
    # 3. the cameras: inside a ball that every rotation keeps in the room, the soup's core or the lattice
    reach = (1.1 if c.family != "lattice" else 0.5) * c.scale
    u = rng.random()
    if c.edge == "room_outside":
        u = 0.85
    c.camt = inside_camera(rng, reach) if u < 0.8 else F.make_camera(rng, c.scale) if u < 0.9 else away_camera(rng, 40 * c.scale)
    c.camt2 = inside_camera(rng, reach)
    # 4. the frame
    c.w, c.h = int(rng.choice(SIDES, p=SIDE_WEIGHTS)), int(rng.choice(SIDES, p=SIDE_WEIGHTS))
    c.spp = int(rng.choice([1, 2, 3], p=[0.2, 0.3, 0.5]))
    # 5. the live mask
    yy, xx = np.meshgrid(np.arange(c.w), np.arange(c.h), indexing="ij")
    c.live = ((yy + xx) % 2 == 0) if rng.random() < 0.5 else (rng.random((c.w, c.h)) < 0.5)
    # 6. the options; rng_table_mb None = left at its default
    c.knobs = {"overlap": int(rng.choice([0, 2])), "slots": int(rng.choice([DEFAULT_SLOTS, c.w * c.h + 17])), "pool": int(rng.integers(0, 2)),
               "resident": int(rng.integers(0, 2)), "primary_resident": int(rng.integers(0, 2)), "rng_table_mb": [None, 0][int(rng.integers(0, 2))],
               "guided": int(rng.integers(0, 4)), "cull": int(rng.random() < 0.8)}
    return c


# ---- expected values: the oracle and the restatements ------------------------------------------------------------------------
class View:
    """One camera of a case: the oracle's frame and the restatements' three masks over its first-bounce rays."""


def product_bih(c):
    if not hasattr(c, "bih"):
        tris = np.zeros(len(c.v), sqt._native.TRI_DTYPE)
        tris["v0"], tris["v1"], tris["v2"], tris["mat"] = c.v[:, 0], c.v[:, 1], c.v[:, 2], c.mat
        c.bih = sqt.BIH(sqt.Mesh.from_arrays(tris, c.mats))
    return c.bih


def records(c):
    """(Level1Cull record, packer scalars, Level1Cover or None, Level1Mirror or None) of the case's scene, and c.plan_on: whether the
    plan's rule turns level-1 culling on under option level1_cull = 1 for a depth-3 path-traced call (sq_plan_call.h, plan_call)."""
    if not hasattr(c, "_records"):
        bih = product_bih(c)
        T, s = R.tables(sqt, bih)
        c._records = (T, s, S.cover(sqt, bih), M5.mirror(sqt, bih))
        c.plan_on = bool(s["level1_on"] and s["n_emitters"] >= 0 and s["nonneg_materials"] and np.isfinite(c.v).all())
    return c._records


def oracle(c):
    if not hasattr(c, "ob"):
        c.ot = oracle_tris_of(O, c.v, c.mats, c.mat)
        c.ob = O.BIH(c.ot)
        c.flat = c.ob.flatten()
    return c.ob


def view(c, second=False, why=None):
    key = "_view2" if second else "_view"
    if not hasattr(c, key) or why is not None:
        T, _, V, M = records(c)
        ob = oracle(c)
        t = View()
        t.cam = O.camera_from_text(c.camt2 if second else c.camt)
        t.avg, t.rgb, _ = ob.render(t.cam, c.spp, c.w, c.h, threads=THREADS)
        t.fb, old, new4, new5 = M5.frame_prediction(sqt, T, V, M, ob, c.flat, t.cam, c.spp, c.w, c.h, why=why)
        t.masks = np.stack([old, new4, new5]) & c.plan_on                # [3, rays]
        setattr(c, key, t)
    return getattr(c, key)


def counts_of(t, sel=None):
    m = t.masks if sel is None else t.masks[:, sel]
    return tuple(int(x) for x in m.sum(1))


# ---- one case on the GPU -----------------------------------------------------------------------------------------------------
DEVICE_ERROR = []      # the first HIP error of this process: after one, no case touches the device again


def run_case(seed):
    """Every check of the seed; returns the list of mismatch messages (empty: all equal).  A refusal is a mismatch."""
    import torch
    F.load_libraries()
    if DEVICE_ERROR:
        raise RuntimeError(f"not run: the device reported an error earlier in this process ({DEVICE_ERROR[0]})")
    c = case(seed)
    bad = []
    records(c)
    t1, t2 = view(c), view(c, second=True)
    cam, cam2 = sqt.camera_from_text(c.camt), sqt.camera_from_text(c.camt2)
    w, h, spp = c.w, c.h, c.spp
    dev = torch.device("cuda", 0)
    ds = sqt.DeviceScene(product_bih(c), 0)
    zero = (0, 0, 0)

    def counters(what, want):
        torch.cuda.synchronize()
        st = ds.stats(reset=True)
        got = (int(st[CULLED]), int(st[STRETCH]), int(st[MIRROR]))
        if got != want:
            bad.append(f"{what}: slots 28, 29, 30 = {got}, predicted {want}")

    def frame(what, avg, rgb, t, live=None):
        avg = avg.cpu().numpy()
        live = np.ones((w, h), bool) if live is None else live
        if not same(avg[live], t.avg[live]):
            bad.append(f"{what}: avg differs in {int((canon(avg) != canon(t.avg)).any(-1)[live].sum())}/{int(live.sum())} pixels")
        elif rgb is not None and not np.array_equal(rgb.cpu().numpy()[live], t.rgb[live]):
            bad.append(f"{what}: rgb8 differs")

    try:
        for k, val in c.knobs.items():
            if val is not None:
                ds.set_option(k, val)
        live = c.live
        for on in (1, 0):
            ds.set_option("level1_cull", on)
            ds.stats(reset=True)
            tag = f"level1_cull {on}"
            # ---- the frame in one call
            avg, rgb = ds.render_rows(cam, spp, w, h)
            counters(f"{tag} render_rows", counts_of(t1) if on else zero)
            frame(f"{tag} render_rows", avg, rgb, t1)
            if ds.last_plan()["level1_cull"] != (on and c.plan_on):
                bad.append(f"{tag}: the plan says level1_cull = {ds.last_plan()['level1_cull']}, its rule {int(on and c.plan_on)}")
            # ---- one sample index at a time
            sums = torch.zeros((w, h, 3), dtype=torch.float32, device=dev)
            for k in range(spp):
                avg, rgb = ds.render_rows_range(cam, spp, w, h, k, k + 1, sums)
                counters(f"{tag} render_rows_range k = {k}", counts_of(t1, t1.fb["k"] == k) if on else zero)
            frame(f"{tag} render_rows_range", avg, rgb, t1)
            # ---- the mask and its complement
            for name, m in (("mask", live), ("complement", ~live)):
                mask = torch.from_numpy(m.astype(np.uint8)).to(dev)
                sums = torch.zeros((w, h, 3), dtype=torch.float32, device=dev)
                avg, rgb = ds.render_rows_masked(cam, spp, w, h, 0, spp, sums, mask=mask)
                counters(f"{tag} render_rows_masked, {name}", counts_of(t1, m[t1.fb["y"], t1.fb["x"]]) if on else zero)
                frame(f"{tag} render_rows_masked, {name}", avg, rgb, t1, m)
            # ---- both cameras in one call
            avg, rgb = ds.render_views([cam, cam2], spp, w, h)
            counters(f"{tag} render_views", tuple(a + b for a, b in zip(counts_of(t1), counts_of(t2))) if on else zero)
            frame(f"{tag} render_views, view 0", avg[0], rgb[0], t1)
            frame(f"{tag} render_views, view 1", avg[1], rgb[1], t2)
            # ---- the camera rays as a query under the frame's seeds
            o, d = ds.camera_rays(cam, w, h)
            rad = ds.raytrace(o, d, seeds=sqt.frame_seeds(spp, w, h, device=dev), samples=spp)
            counters(f"{tag} raytrace", counts_of(t1) if on else zero)
            frame(f"{tag} raytrace", rad.avg, None, t1)
    except sqt.SquiglyError as e:
        if " failed: " in str(e):                                       # a HIP error is no refusal: nothing more runs on this device
            DEVICE_ERROR.append(f"seed {seed}: {e}")
            raise
        bad.append(f"refused: {e}")
    except RuntimeError as e:                                           # torch's own report of a HIP error (a synchronize, a copy)
        if "HIP error" in str(e) or "CUDA error" in str(e):
            DEVICE_ERROR.append(f"seed {seed}: {e}")
        raise
    finally:
        ds.close()
    return bad


def describe(c):
    return (f"seed {c.seed}: {c.family}{' / ' + c.edge if c.edge else ''}, {len(c.v)} tris, scale {c.scale}, rotated {c.rotated}, "
            f"{c.w}x{c.h} @ {c.spp}, {c.knobs}")


def main(budget=240.0, seed=0):
    return F.campaign("fuzz_level1", run_case, budget, seed)


if __name__ == "__main__":
    sys.exit(main(float(sys.argv[1]) if len(sys.argv) > 1 else 240.0, int(sys.argv[2]) if len(sys.argv) > 2 else 0))
