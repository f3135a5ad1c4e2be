"""Transparent padding of a product BIH: taller trees and exact node counts whose expected image is the oracle's image of
the unpadded scene.

A wrapper W inserted above a node X whose traversal box is B has axis a, lmax = B.hi[a], rmin = B.lo[a]; one child is X's
subtree, the other an empty leaf.  Both child boxes are then exactly B (src/BIH.hs:130-141), which every ancestor has
already tested, so W adds no box test and no candidate: in every branch of intersectBIH' (src/BIH.hs:111-123) its result
is X's -- through isClose, through minimumByMay over [near, Nothing], and through `Nothing -> far`.  A ray that visits both
children of W (always, with culling off) pushes one frame for it.

An empty subtree (only empty leaves) can take the empty leaf's place: it never yields a hit either, whatever its boxes.
Hung high in the tree it shifts the breadth-first numbers of the device's branch table (sq_scene_upload), so that the
scene's own deep branches get large indices.

Empty leaves keep link = 0: a kernel that mis-handles an empty leaf reads a real triangle and shows a wrong pixel instead
of faulting.
"""
import ctypes as C
import importlib
import sys

import numpy as np

from kernel_restatements import mt_accepts

N = importlib.import_module("squigly-trace_amd._native")
f32 = np.float32

LEFT, RIGHT = "L", "R"      # which side of a wrapper holds the wrapped subtree (a ray with d[a] > 0 visits the left first)
_EMPTY = ("leaf", 0, 0, -1)


def tree_of(nodes):
    """Pre-order sq_node array -> nested tuples ("leaf", count, first, index) / ("branch", axis, lmax, rmin, left, right, index);
    `index` is the node's pre-order position in the array it came from."""
    def rec(i):
        nd = nodes[i]
        kind = int(nd["kind"])
        if kind & 3 == 3:
            return ("leaf", kind >> 2, int(nd["link"]), i), i + 1
        left, j = rec(i + 1)
        assert j == int(nd["link"])
        right, k = rec(j)
        return ("branch", kind & 3, np.float32(nd["lmax"]), np.float32(nd["rmin"]), left, right, i), k
    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, 10000))
    try:
        t, n = rec(0)
    finally:
        sys.setrecursionlimit(old)
    assert n == len(nodes)
    return t


def empty_tree(n_branches, box, axis=0):
    """A balanced subtree of n_branches branches over empty leaves (every box = box)."""
    if n_branches == 0:
        return _EMPTY
    nl = (n_branches - 1) // 2
    return ("branch", axis, np.float32(box[1][axis]), np.float32(box[0][axis]),
            empty_tree(nl, box, axis), empty_tree(n_branches - 1 - nl, box, axis), -1)


def chain_tree(n_branches, box, axis, near):
    """n_branches branches in a chain over empty leaves (every box = box); each continues on side `near`, so a ray that
    visits that side first holds a frame for every branch of the chain at its bottom."""
    t = _EMPTY
    lmax, rmin = np.float32(box[1][axis]), np.float32(box[0][axis])
    for _ in range(n_branches):
        t = ("branch", axis, lmax, rmin, _EMPTY, t, -1) if near == RIGHT else ("branch", axis, lmax, rmin, t, _EMPTY, -1)
    return t


def _wrap(sub, box, axis, side, other=None):
    other = _EMPTY if other is None else other
    lmax, rmin = np.float32(box[1][axis]), np.float32(box[0][axis])
    l, r = (sub, other) if side == LEFT else (other, sub)
    return ("branch", axis, lmax, rmin, l, r, -1)


def root_chain(k, axes=(0, 1, 2), sides=(LEFT, RIGHT)):
    """k wrappers above the root, cycling through `axes` and `sides` (outermost first)."""
    return {0: [(axes[i % len(axes)], sides[i % len(sides)]) for i in range(k)]}


class PaddedScene:
    """A product BIH with wrappers inserted above chosen nodes.

    wrappers: {pre-order index of the original node: [(axis, side), ...] outermost first}; an entry (axis, side, spec) puts
              an empty subtree in the empty leaf's place: spec ("chain", n, near) = chain_tree, ("balanced", n) = empty_tree
    empties:  {pre-order index: (n_branches, axis, side)}: one more wrapper above that node (above its chain) whose other
              child is an empty subtree of n_branches branches instead of an empty leaf.
    .scene is a ctypes sq_scene over arrays this object keeps alive (DeviceScene, sq_render_f32 and sq_cull_boxes take it)."""

    def __init__(self, bih, wrappers=None, empties=None):
        wrappers, empties = wrappers or {}, empties or {}
        self.base = bih
        root_box = (np.array(bih.scene.root.lo[:], np.float32), np.array(bih.scene.root.hi[:], np.float32))
        tree = tree_of(bih.nodes)
        self.n_wrappers = sum(len(v) for v in wrappers.values()) + len(empties)

        def pad(t, box):                                  # box: the traversal box of t in the padded tree (= in the original)
            if t[0] == "branch":
                _, ax, lmax, rmin, l, r, idx = t
                lbox = (box[0], box[1].copy()); lbox[1][ax] = lmax
                rbox = (box[0].copy(), box[1]); rbox[0][ax] = rmin
                out = ("branch", ax, lmax, rmin, pad(l, lbox), pad(r, rbox), idx)
            else:
                out = t
                idx = t[3]
            for w in reversed(wrappers.get(idx, ())):
                ax, side = w[:2]
                other = None
                if len(w) == 3:                           # (axis, side, ("chain", n, near) | ("balanced", n)): an empty subtree
                    other = chain_tree(w[2][1], box, ax, w[2][2]) if w[2][0] == "chain" else empty_tree(w[2][1], box, ax)
                out = _wrap(out, box, ax, side, other)
            if idx in empties:
                n, ax, side = empties[idx]
                out = _wrap(out, box, ax, side, empty_tree(n, box, ax))
            return out

        old = sys.getrecursionlimit()
        sys.setrecursionlimit(max(old, 10000))
        try:
            padded = pad(tree, root_box)
            rows = []

            def emit(t):
                me = len(rows)
                if t[0] == "leaf":
                    rows.append((3 | (t[1] << 2), 0.0, 0.0, t[2]))
                    return 1
                rows.append(None)
                hl = emit(t[4])
                link = len(rows)
                hr = emit(t[5])
                rows[me] = (t[1], t[2], t[3], link)
                return 1 + max(hl, hr)
            self.height = emit(padded)
        finally:
            sys.setrecursionlimit(old)
        self.nodes = np.array(rows, N.NODE_DTYPE)
        self.tris = bih.tris
        self.mats = bih.materials
        is_leaf = (self.nodes["kind"] & 3) == 3
        self.n_branches = int((~is_leaf).sum())
        self.n_leaves = int(is_leaf.sum())
        self.scene = N.Scene()
        self.scene.root = bih.scene.root
        self.scene.nodes, self.scene.n_nodes = self.nodes.ctypes.data, len(self.nodes)
        self.scene.tris, self.scene.n_tris = (self.tris.ctypes.data if len(self.tris) else None), len(self.tris)
        self.scene.mats, self.scene.n_mats = (self.mats.ctypes.data if len(self.mats) else None), len(self.mats)
        self.scene.height = self.height

    def cull_boxes(self):
        boxes = np.empty((self.scene.n_nodes, 6), np.float32)
        lim = np.empty(3, np.float32)
        N.check(N.lib().sq_cull_boxes(C.byref(self.scene), boxes.ctypes.data, lim.ctypes.data))
        return boxes, tuple(float(x) for x in lim)


def height_with_chain(bih, height):
    """A PaddedScene of `bih` with a root chain that makes the tree exactly `height` tall."""
    return PaddedScene(bih, root_chain(height - bih.height))


def near_side(d):
    """(axis, side) that every ray of directions d visits first: the axis on which all share one sign (the largest
    smallest magnitude), and LEFT for d[axis] > 0, RIGHT for d[axis] < 0."""
    d = np.asarray(d, np.float32)
    ok = [(np.abs(d[:, a]).min(), a) for a in range(3) if (d[:, a] > 0).all() or (d[:, a] < 0).all()]
    assert ok, "the rays share no direction sign on any axis"
    a = max(ok)[1]
    return a, (LEFT if d[0, a] > 0 else RIGHT)


def full_stack_wrappers(bih, height, axis, side, deep=12):
    """Wrappers above the root that make `bih` exactly `height` tall (>= bih.height + 1, deep + 2) and fill the stack of
    every ray that visits `side` of `axis` first: a root chain of height - deep - 2 wrappers that hold their frames while
    the scene is traversed, then one wrapper whose near child is a chain_tree of `deep` branches.  At the bottom of that
    chain such a ray holds height - 1 frames, the most any root-to-leaf path has."""
    other = LEFT if side == RIGHT else RIGHT
    j = height - deep - 2
    assert j >= 0 and deep + 1 >= bih.height, (height, deep, bih.height)
    return [(axis, side)] * j + [(axis, other, ("chain", deep, side))]


def full_stack(bih, height, axis, side, deep=12):
    """PaddedScene of full_stack_wrappers (bih.height itself: the plain tree)."""
    if height == bih.height:
        return PaddedScene(bih)
    return PaddedScene(bih, {0: full_stack_wrappers(bih, height, axis, side, deep)})


def bfs_branch_numbers(nodes):
    """The device's branch numbering (sq_scene_upload): branches breadth-first, stable within a level; -1 for leaves."""
    n = len(nodes)
    depth = np.zeros(n, np.int64)
    leaf = (nodes["kind"] & 3) == 3
    for i in range(n):                                    # pre-order: a parent precedes its children
        if not leaf[i]:
            depth[i + 1] = depth[i] + 1
            depth[int(nodes["link"][i])] = depth[i] + 1
    order = np.lexsort((np.arange(n), depth))
    num = np.full(n, -1, np.int64)
    br = order[~leaf[order]]
    num[br] = np.arange(len(br))
    return num, depth


def _hs_min(x, y):
    return np.where(x <= y, x, y)


def _hs_max(x, y):
    return np.where(x <= y, y, x)


def _slab(lo, hi, o, d):
    """intersectsBB (src/Geometry.hs:166-177): Haskell min / max through NaN, tmax > 0 && tmin < tmax."""
    with np.errstate(all="ignore"):
        df = f32(1) / d
        t1 = (lo - o) * df
        t2 = (hi - o) * df
    mn, mx = _hs_min(t1, t2), _hs_max(t1, t2)
    tmin = _hs_max(_hs_max(mn[:, 0], mn[:, 1]), mn[:, 2])
    tmax = _hs_min(_hs_min(mx[:, 0], mx[:, 1]), mx[:, 2])
    return (tmax > 0) & (tmin < tmax)


def _dist_gt(x, y):
    return ~(x < y) & ~(x == y)


class Mirror:
    """intersectBIH' (src/BIH.hs:101-141, as oracle/sq_oracle.c restates it) over a pre-order sq_node array in fp32 numpy,
    vectorised over rays; intersect() returns (tri, dist, point) per ray, tri = -1 for Nothing.

    It also counts the traversal-stack frames the device kernels hold for each ray (culling off): a FAR frame per branch
    whose near child is being traversed with both children visited, and in its place a COMBINE frame while the far child is
    traversed after a near hit.  .max_held[r] is the most frames ray r holds at a leaf, .visits lists (leaf, ray, held)."""

    def __init__(self, nodes, tris, root_lo, root_hi):
        self.nodes, self.tris = nodes, tris
        self.root = (np.asarray(root_lo, f32), np.asarray(root_hi, f32))

    def intersect(self, o, d):
        o, d = np.asarray(o, f32), np.asarray(d, f32)
        n = len(o)
        self.o, self.d = o, d
        tri = np.full(n, -1, np.int64)
        dist = np.zeros(n, f32)
        pt = np.zeros((n, 3), f32)
        rays = np.arange(n)
        self.max_held = np.zeros(n, np.int64)
        self.visits = []
        held = np.zeros(n, np.int64)
        if (self.nodes["kind"][0] & 3) == 3:              # a single-leaf root is never box-tested (src/BIH.hs:101-109)
            return self._leaf(0, rays, held)
        return self._node(0, self.root, rays, held)

    def _leaf(self, i, rays, held):
        np.maximum.at(self.max_held, rays, held)
        self.visits += [(i, int(r), int(h)) for r, h in zip(rays, held)]
        o, d = self.o[rays], self.d[rays]
        kind, first = int(self.nodes["kind"][i]), int(self.nodes["link"][i])
        tri = np.full(len(rays), -1, np.int64)
        dist = np.zeros(len(rays), f32)
        pt = np.zeros((len(rays), 3), f32)
        for k in range(first, first + (kind >> 2)):
            t = self.tris[k]
            v0, v1, v2 = (np.broadcast_to(np.asarray(t[c], f32), o.shape) for c in ("v0", "v1", "v2"))
            acc, _ = mt_accepts(o, d, v0, v1, v2)
            with np.errstate(all="ignore"):                # t = f * dot(e2, q), point = o + t *^ d (src/Geometry.hs:117-142)
                e1, e2 = v1 - v0, v2 - v0
                s = o - v0
                q = np.stack([s[:, 1] * e1[:, 2] - s[:, 2] * e1[:, 1], s[:, 2] * e1[:, 0] - s[:, 0] * e1[:, 2],
                              s[:, 0] * e1[:, 1] - s[:, 1] * e1[:, 0]], 1)
                h = np.stack([d[:, 1] * e2[:, 2] - d[:, 2] * e2[:, 1], d[:, 2] * e2[:, 0] - d[:, 0] * e2[:, 2],
                              d[:, 0] * e2[:, 1] - d[:, 1] * e2[:, 0]], 1)
                a = (e1[:, 0] * h[:, 0] + e1[:, 1] * h[:, 1]) + e1[:, 2] * h[:, 2]
                tt = (f32(1) / a) * ((e2[:, 0] * q[:, 0] + e2[:, 1] * q[:, 1]) + e2[:, 2] * q[:, 2])
                p = o + tt[:, None] * d
                v = p - o
                dd = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
            take = acc & ((tri < 0) | _dist_gt(dist, dd))  # minimumBy: the earlier one on ties
            tri = np.where(take, k, tri)
            dist = np.where(take, dd, dist)
            pt = np.where(take[:, None], p, pt)
        return tri, dist, pt

    def _node(self, i, box, rays, held):
        n = len(rays)
        tri = np.full(n, -1, np.int64)
        dist = np.zeros(n, f32)
        pt = np.zeros((n, 3), f32)
        if n == 0:
            return tri, dist, pt
        nd = self.nodes[i]
        if (int(nd["kind"]) & 3) == 3:
            return self._leaf(i, rays, held)
        o, d = self.o[rays], self.d[rays]
        inside = _slab(box[0], box[1], o, d)               # src/BIH.hs:112
        ax, lmax, rmin = int(nd["kind"]) & 3, f32(nd["lmax"]), f32(nd["rmin"])
        li, ri = i + 1, int(nd["link"])
        lbox = (box[0], box[1].copy()); lbox[1][ax] = lmax
        rbox = (box[0].copy(), box[1]); rbox[0][ax] = rmin
        iL = inside & _slab(lbox[0], lbox[1], o, d)
        iR = inside & _slab(rbox[0], rbox[1], o, d)

        def put(sel, res):
            tri[sel], dist[sel], pt[sel] = res

        both = iL & iR
        l2r = d[:, ax] > 0                                 # src/BIH.hs:127
        for go_left_first in (True, False):
            sel = np.nonzero(both & (l2r == go_left_first))[0]
            if not len(sel):
                continue
            near = self._node(li, lbox, rays[sel], held[sel] + 1) if go_left_first else self._node(ri, rbox, rays[sel], held[sel] + 1)
            put(sel, near)
            hit = near[0] >= 0
            p = near[2][:, ax]
            close = (p < rmin) if go_left_first else (p > lmax)   # isClose, src/BIH.hs:121-123
            far_sel = sel[~hit | (hit & ~close)]
            nh = hit[np.searchsorted(sel, far_sel)]
            fh = held[far_sel] + nh                        # COMBINE(near) replaces FAR while the far child runs
            far = self._node(ri, rbox, rays[far_sel], fh) if go_left_first else self._node(li, lbox, rays[far_sel], fh)
            # near missed: far's result (src/BIH.hs:116); near hit: minimumByMay [near, far] (src/BIH.hs:115,120)
            use_far = (~nh & True) | (nh & (far[0] >= 0) & _dist_gt(dist[far_sel], far[1]))
            put(far_sel[use_far], tuple(x[use_far] for x in far))
        only_l = np.nonzero(iL & ~iR)[0]
        put(only_l, self._node(li, lbox, rays[only_l], held[only_l]))      # src/BIH.hs:117
        only_r = np.nonzero(iR & ~iL)[0]
        put(only_r, self._node(ri, rbox, rays[only_r], held[only_r]))      # src/BIH.hs:118
        return tri, dist, pt
