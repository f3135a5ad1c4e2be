"""Resident-scene rendering on one MI355X: the scene is uploaded once, frames stay in HBM.

PyTorch is used only for device memory and streams (plumbing); every pixel is produced by the HIP
kernels in csrc/sq_device.hip through the C-ABI of include/squigly_hip.h.
"""
import collections
import ctypes as C

import torch

from . import _native as N
from . import _plumbing as P
from .scene import Owner

Hits = collections.namedtuple("Hits", ["tri", "dist", "point"])
Hits.__doc__ = """Results of DeviceScene.intersect: Maybe Intersection (src/Geometry.hs:71-75) per ray; tri = -1 is Nothing."""

Radiance = collections.namedtuple("Radiance", ["sum", "avg", "rgb"])
Radiance.__doc__ = """Results of DeviceScene.raytrace per ray: the fold of its sample radiances, (1 / k_end) * sum, and its tonemap."""


# The largest frame one call takes (include/squigly_hip.h): pixel indices are 32-bit, and the wavefront form's
# active-pixel list and ray queue hold while a call has at most 2^29 pixels.
MAX_CALL_PIXELS = 2 ** 31 - 1
MAX_WAVEFRONT_PIXELS = 2 ** 29


def frame_size_error(rows, h, views=1, wavefront=False):
    """The library's refusal of a call of views x rows x h pixels, word for word, or None when the size is accepted.
    wavefront: the call takes the wavefront form (option "variant" = 2; a cast frame only with option "cast_wavefront" = 1)."""
    rows, h, views = int(rows), int(h), int(views)
    if rows <= 0 or h <= 0 or views <= 0:
        return None
    pixels = views * rows * h
    what = f"{views} views of {rows} x {h} pixels" if views > 1 else f"{rows} x {h} pixels"
    if pixels > MAX_CALL_PIXELS:
        return f"{what} exceed 2^31 - 1 pixels in one call"
    if wavefront and pixels > MAX_WAVEFRONT_PIXELS:
        other = "variant 1" if views > 1 else "variant 1 and cast frames"
        return f"{what} exceed 2^29 pixels in one call of the wavefront form ({other} take{'s' if views > 1 else ''} 2^31 - 1)"
    return None


def _check_frame_size(dscene, rows, h, cast, views=1):
    """SquiglyError, before anything is allocated, for a frame the library would refuse for its size."""
    msg = frame_size_error(rows, h, views, getattr(dscene, "_variant", 2) != 1 and (not cast or getattr(dscene, "_cast_wavefront", 0) != 0))
    if msg:
        raise N.SquiglyError(msg)


def _ray_shape(origins, directions):
    """The common [..., 3] shape of a query's origins and directions; SquiglyError before any device work otherwise."""
    shapes = []
    for name, a in (("origins", origins), ("directions", directions)):
        shape = tuple(a.shape) if hasattr(a, "shape") else tuple(torch.as_tensor(a).shape)
        if len(shape) < 1 or shape[-1] != 3:
            raise N.SquiglyError(f"{name} must have shape [..., 3], got {shape}")
        shapes.append(shape)
    if shapes[0] != shapes[1]:
        raise N.SquiglyError(f"origins {shapes[0]} and directions {shapes[1]} must have the same shape")
    return shapes[0]


def frame_seeds(samples, w, h, shard=(None, 0, 1), device=None):
    """The seed bases of a frame's pixels (src/Lib.hs:85): an int64 tensor [rows, h] holding samples * (x + y * w) for the global
    row y of every local row of the shard (sq_shard_global_row) and every column x.  With them
    ds.raytrace(*ds.camera_rays(cam, w, h, shard), seeds=frame_seeds(samples, w, h, shard), samples=samples) is the frame.
    Pure integer arithmetic: device=None builds the tensor on the CPU."""
    samples, w, h = int(samples), int(w), int(h)
    if samples < 1 or w < 1 or h < 1:
        raise N.SquiglyError(f"samples, width and height must be positive (got {samples}, {w}, {h})")
    rb, si, ns = P.shard_ints(w, shard)
    if rb <= 0 or ns <= 0 or si < 0 or si >= ns:     # sq_shard_rows' own refusal, restated: no library's device side is needed here
        raise N.SquiglyError(f"bad shard {shard}")
    blocks = torch.arange(si, (w + rb - 1) // rb, ns, dtype=torch.int64, device=device)       # this shard's row blocks
    y = (blocks[:, None] * rb + torch.arange(rb, dtype=torch.int64, device=device)[None, :]).reshape(-1)
    y = y[y < w]                                                                             # the image's last block may be short
    x = torch.arange(h, dtype=torch.int64, device=device)
    return samples * (x[None, :] + y[:, None] * w)


def _lead_count(lead):
    n = 1
    for v in lead:
        n *= int(v)
    return n


# The state a frame carries from call to call, per pixel [rows, h]: name -> (trailing shape, dtype)
_STATE = {"sums": ((3,), torch.float32), "mask": ((), torch.uint8), "sums2": ((3,), torch.float32), "counts": ((), torch.int32)}


class DeviceScene(Owner):
    """A BIH uploaded to one GPU (sq_scene_upload)."""
    _free = "sq_scene_free"

    def __init__(self, bih, device=0):
        self.bih = bih                      # keeps the host arrays alive
        self.device = int(device)
        h = C.c_void_p()
        N.check(N.lib().sq_scene_upload(C.byref(bih.scene), self.device, C.byref(h)))
        self._h = h

    def set_option(self, key, value):
        N.check(N.lib().sq_set_option(self._h, key.encode(), int(value)))
        if key == "variant":
            self._variant = int(value)       # which size limit a frame has (_check_frame_size)
        if key == "cast_wavefront":
            self._cast_wavefront = int(bool(value))

    def set_lights(self, lights, stream=None):
        """The point lights of the scene's cast frames and raycast queries (sq_scene_set_lights), in the order their terms are
        added.  lights: an array-like [n, 6] (pos, power), or a sequence of (pos, power) pairs with power a scalar or three
        numbers; None restores the reference's light (REFERENCE_LIGHT).  The update is enqueued on `stream` like a frame, and
        the argument may be reused as soon as the call returns."""
        table = None if lights is None else N.lights_array(lights)      # shape and count errors come before any device work
        _, st = P.call_stream(self.device, stream)
        N.check(N.lib().sq_scene_set_lights(self._h, None if table is None else table.ctypes.data, 0 if table is None else len(table),
                                            P.stream_ptr(st)))

    @property
    def lights(self):
        """The scene's lights as a float32 numpy array [n, 6] (pos, power), from the library's copy (sq_scene_get_lights)."""
        import numpy as np
        n = N.count(N.lib().sq_scene_get_lights(self._h, None, 0))
        out = np.empty((n, 6), np.float32)
        N.lib().sq_scene_get_lights(self._h, out.ctypes.data, n)
        return out

    def set_depth(self, depth):
        """The path depth D of the scene's path-traced frames and raytrace queries (sq_scene_set_depth): a path is D rays long,
        1 <= D <= 8; 3 is the reference's (src/Lib.hs:129) and every scene's until set.  Host state that the next call reads:
        nothing is enqueued.  Cast frames and raycast ignore it."""
        d = N.depth_value(depth)                                        # refused before any device work
        N.check(N.lib().sq_scene_set_depth(self._h, d))

    @property
    def depth(self):
        """The scene's path depth (sq_scene_get_depth)."""
        return int(N.count(N.lib().sq_scene_get_depth(self._h)))

    def set_sky(self, up, down=None):
        """The sky of the scene's path-traced frames and raytrace queries (sq_scene_set_sky): the radiance of a ray that leaves
        the scene, `up` seen looking along +z and `down` along -z (three numbers each; down = None: a constant sky, down = up).
        set_sky(None) resets the scene to no sky, the reference's black.  Host state that the next call reads: nothing is
        enqueued.  Cast frames and raycast ignore it."""
        if up is None:
            if down is not None:
                raise N.SquiglyError("set_sky(None) resets the sky and takes no down")
            N.check(N.lib().sq_scene_set_sky(self._h, None))
            return
        table = N.sky_value(up, down)                                   # refused before any device work
        N.check(N.lib().sq_scene_set_sky(self._h, table.ctypes.data))

    @property
    def sky(self):
        """The scene's sky (sq_scene_get_sky): None, or (up, down), two tuples of three floats."""
        import numpy as np
        out = np.zeros((2, 3), np.float32)
        r = N.count(N.lib().sq_scene_get_sky(self._h, out.ctypes.data))
        return None if r == 0 else (tuple(float(v) for v in out[0]), tuple(float(v) for v in out[1]))

    def rng_table(self, first=0, count=0):
        """sq_scene_rng_table: (seeds the scene's table of generator words holds, its entries [first, first + count) as a uint32
        numpy array [count, 3])."""
        import numpy as np
        out = np.empty((int(count), 3), np.uint32)
        return int(N.count(N.lib().sq_scene_rng_table(self._h, int(first), int(count), out.ctypes.data))), out

    def _outputs(self, w, h, shard, want_avg, want_rgb, stream, out_avg, out_rgb, views=None, cast=False, frame=True):
        """(sq_shard, rows, out_avg, out_rgb, stream) of a render_rows* call: the shard's row count, the output tensors
        (allocated unless given or not wanted) and the stream (default: the device's current one).  views: the tensors get a
        leading dimension of that many views (render_views)."""
        sh, rows = P.shard_rows(w, shard)
        if frame:                              # frame: a render call (camera_rays has no limit but memory)
            _check_frame_size(self, rows, h, cast, 1 if views is None else views)
        shape = (rows, h, 3) if views is None else (views, rows, h, 3)
        dev, st = P.call_stream(self.device, stream)
        with torch.cuda.stream(st):      # allocated in the order of the call's stream: a block another stream still has work on is not taken
            if want_avg and out_avg is None:
                out_avg = torch.empty(shape, dtype=torch.float32, device=dev)
            if want_rgb and out_rgb is None:
                out_rgb = torch.empty(shape, dtype=torch.uint8, device=dev)
        return sh, rows, out_avg, out_rgb, st

    def _frame_tensor(self, name, t, shape, dtype, says=None):
        """t if it is a contiguous `dtype` tensor of `shape` on this device; SquiglyError otherwise (P.tensor)."""
        return P.tensor(name, t, shape, dtype, torch.device("cuda", self.device), says)

    def _rows_call(self, what, w, h, cast, shard, want_avg, want_rgb, stream, out_avg, out_rgb, says=None, **state):
        """What the render_rows* methods do before their C call: _outputs, then, for the two that carry a fold, the refusal of a
        missing sums in the name of the method `what`, and every state tensor given (sums, mask, sums2, counts, in that order)
        held to the shard's shape.  Returns (sq_shard, out_avg, out_rgb, stream)."""
        sh, rows, out_avg, out_rgb, st = self._outputs(w, h, shard, want_avg, want_rgb, stream, out_avg, out_rgb, cast=cast)
        if "sums" in state and state["sums"] is None:
            raise N.SquiglyError(f"{what} needs a sums tensor")
        for name, t in state.items():
            if t is not None:
                self._frame_tensor(name, t, (rows, h) + _STATE[name][0], _STATE[name][1], says)
        return sh, out_avg, out_rgb, st

    def render_rows(self, cam, samples, w, h, cast=False, shard=(None, 0, 1), want_avg=True, want_rgb=True,
                    stream=None, out_avg=None, out_rgb=None):
        """Enqueue the render of this shard's rows; returns (avg, rgb) CUDA tensors [rows, h, 3].

        shard = (row_block, shard_index, n_shards); row_block None = all rows in one block.
        """
        sh, out_avg, out_rgb, st = self._rows_call("render_rows", w, h, cast, shard, want_avg, want_rgb, stream, out_avg, out_rgb)
        N.check(N.lib().sq_render_rows_device(
            self._h, C.byref(cam), samples, w, h, int(bool(cast)), sh, P.ptr(out_avg), P.ptr(out_rgb), P.stream_ptr(st)))
        return out_avg, out_rgb

    def render_rows_range(self, cam, samples, w, h, k_begin, k_end, sums, cast=False, shard=(None, 0, 1), want_avg=True,
                          want_rgb=True, stream=None, out_avg=None, out_rgb=None):
        """Enqueue the samples [k_begin, k_end) of the `samples`-sample frame (sq_render_rows_device_range); returns (avg, rgb)
        of the k_end samples folded so far.

        sums: float32 CUDA tensor [rows, h, 3] on this device, the per-pixel fold over [0, k_begin) on entry (ignored when
        k_begin == 0) and over [0, k_end) once the stream gets there.
        """
        sh, out_avg, out_rgb, st = self._rows_call("render_rows_range", w, h, cast, shard, want_avg, want_rgb, stream, out_avg, out_rgb,
                                                   says="float32", sums=sums)
        N.check(N.lib().sq_render_rows_device_range(
            self._h, C.byref(cam), samples, w, h, int(bool(cast)), sh, int(k_begin), int(k_end), sums.data_ptr(),
            P.ptr(out_avg), P.ptr(out_rgb), P.stream_ptr(st)))
        return out_avg, out_rgb

    def render_rows_masked(self, cam, samples, w, h, k_begin, k_end, sums, mask=None, sums2=None, counts=None, cast=False,
                           shard=(None, 0, 1), want_avg=True, want_rgb=True, stream=None, out_avg=None, out_rgb=None):
        """render_rows_range for the live pixels only (sq_render_rows_device_masked); returns (avg, rgb).

        mask: uint8 CUDA tensor [rows, h], a pixel is rendered iff its byte is not 0 (None = every pixel) and, when counts is
        given and k_begin > 0, counts[pixel] == k_begin.  sums2: float32 [rows, h, 3], the fold of r * r carried like sums.
        counts: int32 [rows, h], set to k_end for the pixels rendered.  Pixels that are not rendered keep what every buffer
        holds -- avg and rgb too, so pass out_avg / out_rgb to keep a picture across calls (fresh ones are zero-filled).
        With mask, sums2 and counts all None this is render_rows_range.
        """
        given_avg, given_rgb = out_avg is not None, out_rgb is not None
        sh, out_avg, out_rgb, st = self._rows_call("render_rows_masked", w, h, cast, shard, want_avg, want_rgb, stream, out_avg, out_rgb,
                                                   sums=sums, mask=mask, sums2=sums2, counts=counts)
        if mask is not None or sums2 is not None or counts is not None:      # a masked call clears nothing: no stale memory in fresh outputs
            with torch.cuda.stream(st):
                if out_avg is not None and not given_avg:
                    out_avg.zero_()
                if out_rgb is not None and not given_rgb:
                    out_rgb.zero_()
        N.check(N.lib().sq_render_rows_device_masked(
            self._h, C.byref(cam), samples, w, h, int(bool(cast)), sh, int(k_begin), int(k_end), P.ptr(mask), sums.data_ptr(),
            P.ptr(sums2), P.ptr(counts), P.ptr(out_avg), P.ptr(out_rgb), P.stream_ptr(st)))
        return out_avg, out_rgb

    def adaptive_update(self, sums, sums2, counts, mask, tol, eps, stream=None):
        """The built-in stopping rule (sq_adaptive_update_device) on the pixels whose mask byte is set: a converged pixel's byte
        is cleared.  Returns the number of pixels still live (waits for the stream).  A heuristic: see include/squigly_hip.h."""
        dev, st = P.call_stream(self.device, stream)
        shape = tuple(mask.shape)
        for name, t in (("mask", mask), ("sums", sums), ("sums2", sums2), ("counts", counts)):
            self._frame_tensor(name, t, shape + _STATE[name][0], _STATE[name][1])
        if mask.numel() == 0:
            return 0
        with torch.cuda.stream(st):
            live = torch.empty(1, dtype=torch.int32, device=dev)
            N.check(N.lib().sq_adaptive_update_device(self._h, int(mask.numel()), sums.data_ptr(), sums2.data_ptr(), counts.data_ptr(),
                                                      float(tol), float(eps), mask.data_ptr(), live.data_ptr(), P.stream_ptr(st)))
            st.synchronize()
            return int(live.item())

    def render_views(self, cams, samples, w, h, cast=False, shard=(None, 0, 1), k_begin=0, k_end=None, sums=None, want_avg=True,
                     want_rgb=True, stream=None, out_avg=None, out_rgb=None):
        """Enqueue the frames of many cameras in one call (sq_render_views_device); returns (avg, rgb) CUDA tensors
        [n_views, rows, h, 3].  View i is bit for bit render_rows_range of cams[i] with the same other arguments.

        k_begin, k_end: the sample range, [0, samples) by default (k_end None = samples).  sums: float32 CUDA tensor
        [n_views, rows, h, 3] carrying the per-pixel fold as in render_rows_range; it may be None only for [0, samples).
        """
        cams = list(cams)
        if not cams:
            raise ValueError("render_views needs at least one camera")
        n = len(cams)
        k_end = int(samples) if k_end is None else int(k_end)
        sh, rows, out_avg, out_rgb, st = self._outputs(w, h, shard, want_avg, want_rgb, stream, out_avg, out_rgb, views=n, cast=cast)
        if sums is not None:
            self._frame_tensor("sums", sums, (n, rows, h, 3), torch.float32, says="float32")
        table = (N.Camera * n)(*cams)
        N.check(N.lib().sq_render_views_device(
            self._h, table, n, samples, w, h, int(bool(cast)), sh, int(k_begin), k_end, P.ptr(sums), P.ptr(out_avg), P.ptr(out_rgb),
            P.stream_ptr(st)))
        return out_avg, out_rgb

    def intersect(self, origins, directions, want_dist=True, want_point=True, stream=None, out=None):
        """intersectBIH of each ray (sq_intersect_rays_device); returns Hits(tri, dist, point) CUDA tensors, enqueued on `stream`.

        origins, directions: any [..., 3] arrays of one shape (numpy, a CPU or CUDA tensor, lists); they are converted to
        contiguous float32 on this device, so float64 input is rounded to the nearest float32 first.  tri (int32) and dist
        (float32) have the leading shape, point (float32) the whole shape; tri is the index into bih.tris (leaf order), -1 on a
        miss, where dist = +inf and point = (+0, +0, +0).  want_dist / want_point = False leave that field None.
        out: Hits whose tensors (contiguous, right shape and dtype, on this device; None = allocate) receive the results.
        """
        shape = _ray_shape(origins, directions)
        dev, st = P.call_stream(self.device, stream)
        lead = shape[:-1]
        out = Hits(*(out if out is not None else (None, None, None)))
        for name, t, want, tshape, dtype in (("tri", out.tri, True, lead, torch.int32), ("dist", out.dist, want_dist, lead, torch.float32),
                                             ("point", out.point, want_point, shape, torch.float32)):
            if t is not None and want:
                P.tensor(f"out.{name}", t, tshape, dtype, dev)
        with torch.cuda.stream(st):      # temporaries are allocated and freed in the order of the call's stream
            o, d = P.rays_in(dev, origins, directions)
            tri = out.tri if out.tri is not None else torch.empty(lead, dtype=torch.int32, device=dev)
            dist = (out.dist if out.dist is not None else torch.empty(lead, dtype=torch.float32, device=dev)) if want_dist else None
            point = (out.point if out.point is not None else torch.empty(shape, dtype=torch.float32, device=dev)) if want_point else None
            N.check(N.lib().sq_intersect_rays_device(self._h, o.data_ptr(), d.data_ptr(), int(o.numel() // 3), tri.data_ptr(), P.ptr(dist),
                                                     P.ptr(point), P.stream_ptr(st)))
        return Hits(tri, dist, point)

    def camera_rays(self, cam, w, h, shard=(None, 0, 1), stream=None):
        """The primary ray of every pixel of the shard, as the renderer traces it (sq_camera_rays_device): (origins,
        directions) float32 CUDA tensors [rows, h, 3].  ds.intersect(*ds.camera_rays(cam, w, h)) is the frame's depth and
        triangle-id buffer."""
        sh, rows, _, _, st = self._outputs(w, h, shard, False, False, stream, None, None, frame=False)
        dev = torch.device("cuda", self.device)
        with torch.cuda.stream(st):      # as in _outputs: the rays are allocated in the order of the call's stream
            o = torch.empty((rows, h, 3), dtype=torch.float32, device=dev)
            d = torch.empty((rows, h, 3), dtype=torch.float32, device=dev)
        N.check(N.lib().sq_camera_rays_device(self._h, C.byref(cam), int(w), int(h), sh, o.data_ptr(), d.data_ptr(), P.stream_ptr(st)))
        return o, d

    def guides(self, cam, w, h, shard=(None, 0, 1), stream=None):
        """What the denoiser is guided by (denoise.py): Guides(tri, point, normal, surf, emit) of every pixel's first hit, from
        camera_rays + intersect and gathers from the scene's triangle and material arrays.  tri = -1 where nothing is hit, and the
        other fields are zeros there.  Held to the oracle's first hits and triangles bit for bit on random scenes (tests/fuzz_lens.py)."""
        from .denoise import scene_guides
        return scene_guides(self, cam, w, h, shard, stream)

    def lens_rays(self, cam, lens, samples, subrays, w, h, shard=(None, 0, 1), r_range=None, stream=None):
        """The jittered, thin-lens sub-rays of every pixel of the shard (lens.py, sq_lens_rays_device): (origins, directions, seeds),
        float32 CUDA tensors [nb, rows, h, 3] and int64 [nb, rows, h] for the sub-rays r_range (default: all `subrays`)."""
        from .lens import lens_rays
        return lens_rays(self, cam, lens, samples, subrays, w, h, shard, r_range, stream)

    def render_lens(self, cam, lens, samples, subrays, w, h, shard=(None, 0, 1), r_range=None, sums=None, want_sum2=False,
                    want_avg=True, want_rgb=True, work_mb=None, stream=None):
        """The anti-aliased, depth-of-field frame (lens.py, sq_lens_render_device): `subrays` primary rays per pixel, samples /
        subrays samples on each, folded in sub-ray order; returns LensFrame(sum, sum2, avg, rgb).  See lens.render_lens."""
        from .lens import render_lens
        return render_lens(self, cam, lens, samples, subrays, w, h, shard, r_range, sums, want_sum2, want_avg, want_rgb, work_mb, stream)

    def live_pixels(self, mask, counts, r_begin, stream=None):
        """The live list of a masked lens step (mlens.py, sq_mlens_live_device): (index, n_live), int32 CUDA tensors -- the live
        pixels in ascending order in the first n_live entries of index, and n_live itself, [1].  See mlens.live_pixels."""
        from .mlens import live_pixels
        return live_pixels(self, mask, counts, r_begin, stream)

    def render_lens_masked(self, cam, lens, samples, subrays, w, h, r_begin, r_end, sums, index, n_live, sums2=None, counts=None,
                           shard=(None, 0, 1), work_mb=None, out_avg=None, out_rgb=None, stream=None):
        """render_lens for the listed pixels only (mlens.py, sq_mlens_render_device): the sub-rays [r_begin, r_end) of the first
        n_live pixels of `index`, folded into their sums, sums2 and counts (in sub-rays); a pixel that is not listed costs no ray
        and keeps what every buffer holds.  Returns (out_avg, out_rgb).  See mlens.render_lens_masked."""
        from .mlens import render_lens_masked
        return render_lens_masked(self, cam, lens, samples, subrays, w, h, r_begin, r_end, sums, index, n_live, sums2, counts, shard,
                                  work_mb, out_avg, out_rgb, stream)

    def shutter_rays(self, motion, lens, samples, subrays, w, h, shard=(None, 0, 1), r_range=None, stream=None):
        """lens_rays under a camera that moves during the exposure (shutter.py, sq_shutter_rays_device): sub-ray r of a pixel is
        made under the pose of its own instant of `motion` (a Motion).  See shutter.shutter_rays."""
        from .shutter import shutter_rays
        return shutter_rays(self, motion, lens, samples, subrays, w, h, shard, r_range, stream)

    def render_shutter(self, motion, lens, samples, subrays, w, h, shard=(None, 0, 1), r_range=None, sums=None, want_sum2=False,
                       want_avg=True, want_rgb=True, work_mb=None, stream=None):
        """The motion-blurred frame (shutter.py, sq_shutter_render_device): render_lens whose `subrays` primary rays per pixel are
        as many consecutive instants of `motion`; returns LensFrame(sum, sum2, avg, rgb).  See shutter.render_shutter."""
        from .shutter import render_shutter
        return render_shutter(self, motion, lens, samples, subrays, w, h, shard, r_range, sums, want_sum2, want_avg, want_rgb, work_mb,
                              stream)

    def render_shutter_masked(self, motion, lens, samples, subrays, w, h, r_begin, r_end, sums, index, n_live, sums2=None, counts=None,
                              shard=(None, 0, 1), work_mb=None, out_avg=None, out_rgb=None, stream=None):
        """render_lens_masked under a moving camera (shutter.py, sq_shutter_render_device with the list of live_pixels).  Returns
        (out_avg, out_rgb).  See shutter.render_shutter_masked."""
        from .shutter import render_shutter_masked
        return render_shutter_masked(self, motion, lens, samples, subrays, w, h, r_begin, r_end, sums, index, n_live, sums2, counts,
                                     shard, work_mb, out_avg, out_rgb, stream)

    def raytrace(self, origins, directions, seeds=None, samples=1, k_range=None, sums=None, want_avg=True, want_rgb=False,
                 stream=None):
        """Lib.raytrace of each ray (sq_raytrace_rays_device): returns Radiance(sum, avg, rgb) CUDA tensors, enqueued on `stream`.

        origins, directions: any [..., 3] arrays of one shape, converted as in `intersect` (float64 is rounded to float32 first).
        seeds: int64 [...] seed bases; sample k of a ray draws from mkTFGen (seed + k).  None means samples * i for the i-th ray in
        row-major order -- distinct generators for every sample of the batch, NOT a frame's rule unless w == h (see frame_seeds).
        k_range = (k_begin, k_end): the samples folded by this call, (0, samples) by default.  sums: float32 CUDA tensor [..., 3]
        carrying the fold as in render_rows_range; required when k_begin > 0, updated in place, allocated otherwise.
        sum is the left fold of the sample radiances, avg = (1 / k_end) * sum (None unless want_avg), rgb its tonemap (uint8, None
        unless want_rgb).  A ray that hits nothing gets zeros.
        """
        shape = _ray_shape(origins, directions)
        lead = shape[:-1]
        n = _lead_count(lead)
        samples = int(samples)
        if samples < 1:
            raise N.SquiglyError(f"samples must be positive, got {samples}")
        k_begin, k_end = (0, samples) if k_range is None else (int(k_range[0]), int(k_range[1]))
        if k_begin < 0 or k_end <= k_begin or k_end >= 2 ** 31:
            raise N.SquiglyError(f"bad sample range [{k_begin}, {k_end}) (need 0 <= k_begin < k_end)")
        if seeds is not None:
            sshape = tuple(seeds.shape) if hasattr(seeds, "shape") else tuple(torch.as_tensor(seeds).shape)
            if sshape != tuple(lead):
                raise N.SquiglyError(f"seeds must have shape {tuple(lead)}, got {sshape}")
            sdtype = seeds.dtype if isinstance(seeds, torch.Tensor) else torch.as_tensor(seeds).dtype
            if sdtype not in (torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8):
                raise N.SquiglyError(f"seeds must be integers (int64), got {sdtype}")
        if sums is None:
            if k_begin > 0:
                raise N.SquiglyError("raytrace needs the sums of the samples [0, k_begin) when k_range starts above 0")
        else:
            if not isinstance(sums, torch.Tensor):
                raise N.SquiglyError("sums must be a CUDA tensor: it is updated in place")
            self._frame_tensor("sums", sums, shape, torch.float32)
        dev, st = P.call_stream(self.device, stream)
        with torch.cuda.stream(st):      # temporaries are allocated and freed in the order of the call's stream
            o, d = P.rays_in(dev, origins, directions)
            if seeds is None:
                sd = (samples * torch.arange(n, dtype=torch.int64, device=dev)).reshape(lead)
            else:
                sd = torch.as_tensor(seeds, device=dev).to(torch.int64).contiguous()
            if sums is None:
                sums = torch.empty(shape, dtype=torch.float32, device=dev)
            avg = torch.empty(shape, dtype=torch.float32, device=dev) if want_avg else None
            rgb = torch.empty(shape, dtype=torch.uint8, device=dev) if want_rgb else None
            N.check(N.lib().sq_raytrace_rays_device(self._h, o.data_ptr(), d.data_ptr(), sd.data_ptr(), n, k_begin, k_end, sums.data_ptr(),
                                                    P.ptr(avg), P.ptr(rgb), P.stream_ptr(st)))
        return Radiance(sums, avg, rgb)

    def raycast(self, origins, directions, stream=None):
        """Lib.raycast of each ray (sq_raycast_rays_device) under the scene's lights (set_lights; the reference's light at
        (0, 3, -1) unless set): a float32 CUDA tensor [..., 3], zeros for a miss or a point every light is shadowed at.  origins, directions as in `intersect`."""
        shape = _ray_shape(origins, directions)
        dev, st = P.call_stream(self.device, stream)
        with torch.cuda.stream(st):
            o, d = P.rays_in(dev, origins, directions)
            rad = torch.empty(shape, dtype=torch.float32, device=dev)
            N.check(N.lib().sq_raycast_rays_device(self._h, o.data_ptr(), d.data_ptr(), _lead_count(shape[:-1]), rad.data_ptr(),
                                                   P.stream_ptr(st)))
        return rad

    def enable_timing(self, on=True):
        """Bracket every launch of the dominant kernel with hipEvents (read back by kernel_timing)."""
        self.set_option("timing", int(bool(on)))

    def kernel_timing(self):
        """(average ms per launch of the dominant kernel, launches, kernel name) since the last reset."""
        ms, n, name = C.c_double(), C.c_int64(), C.c_char_p()
        N.check(N.lib().sq_kernel_timing(self._h, C.byref(ms), C.byref(n), C.byref(name)))
        return ms.value, n.value, (name.value or b"").decode()

    def stats(self, reset=False):
        """Cumulative trace-kernel statistics: [rays traced, profile counters...] (synchronises); slots 28, 29 and 30 = the
        first-bounce rays that level-1 culling (option "level1_cull") did not queue: by its conditions (1)-(3), by condition (4) alone and by
        condition (5) alone."""
        out = (C.c_uint64 * 32)()
        N.check(N.lib().sq_get_stats(self._h, out, 32, int(reset)))
        return [int(v) for v in out]

    def last_plan(self):
        """sq_last_plan: what the last render_rows call chose -- trace form ("resident", "streaming_six_wave",
        "streaming_plain" or "per_pixel"), stack word bytes, workgroups per CU, LDS sizes, ... -- as a dict."""
        p = N.Plan()
        N.check(N.lib().sq_last_plan(self._h, C.byref(p)))
        d = {name: int(getattr(p, name)) for name, _ in N.Plan._fields_}
        d["trace_form"] = N.TRACE_FORMS[d["trace_form"]]
        d["primary_form"] = N.PRIMARY_FORMS[d["primary_form"]]
        return d

    def reset_timing(self):
        N.lib().sq_kernel_timing_reset(self._h)

    close = Owner._release


SCENE_SKY = object()     # sky= of Progressive / Adaptive: a fresh frame, which runs under the scene's sky whatever it is


def _sky_bits(sky):
    """A sky as bytes, so that two skies are the same when their bits are (a NaN component equals itself); None = no sky."""
    pair = N.sky_pair(sky)
    return None if pair is None else pair.tobytes()


# What a path-traced frame runs under besides its own arguments, in the order it is checked: the attribute (of the scene and of the
# frame), what the constructor takes for "a fresh frame", what two values are the same by, how a refusal words the frame's value and
# the scene's, and the call that makes the scene match a checkpoint.
_UNDER = (("depth", None, N.depth_value, lambda d: f"depth {int(d)}", lambda d: f"depth {d}", lambda d: f"set_depth({int(d)})"),
          ("sky", SCENE_SKY, _sky_bits, lambda s: f"the sky {s!r}", repr, lambda s: "set_sky"))


class _Frame:
    """What Progressive and Adaptive share: the shard's rows, the size check, the depth and the sky the frame runs under, and
    the adoption of a checkpoint's tensors."""

    def _begin(self, dscene, cam, samples, w, h, cast, shard, **under):
        """Sets the frame's fields and returns its row count.  under: depth and sky as the constructor got them -- what a checkpoint
        carried (for the depth, None is also a checkpoint from before depths existed, which is the scene's own).  The frame runs
        under the scene's; SquiglyError when a checkpoint was rendered under another.  A cast frame has no paths: it ignores the
        depth and the sky, and its fields are None."""
        _, rows = P.shard_rows(w, shard)
        _check_frame_size(dscene, rows, h, cast)
        for name, fresh, key, mine, theirs, fix in _UNDER:
            have = None if cast else getattr(dscene, name)
            if not cast and under[name] is not fresh and key(under[name]) != key(have):
                raise N.SquiglyError(f"the checkpoint was rendered under {mine(under[name])}, the scene has {theirs(have)}: "
                                     f"{fix(under[name])} first")
            setattr(self, name, have)
        self.dscene, self.cam, self.samples, self.w, self.h = dscene, cam, samples, int(w), int(h)
        self.cast, self.shard = bool(cast), shard
        self._dev = torch.device("cuda", dscene.device)
        return rows

    def _unchanged(self):
        """SquiglyError when the scene's depth or sky is no longer what the frame was begun under."""
        for name, _, key, mine, theirs, _ in () if self.cast else _UNDER:
            was, have = getattr(self, name), getattr(self.dscene, name)
            if key(have) != key(was):
                raise N.SquiglyError(f"the frame was begun under {mine(was)}, the scene now has {theirs(have)}")

    def _adopt(self, name, t, shape, dtype, fill=None):
        """A checkpoint's tensor: a matching CUDA tensor as it is; anything else (a host copy) is copied to the device.  None: a
        new tensor, filled with `fill` unless that is None."""
        if t is None:
            return torch.empty(shape, dtype=dtype, device=self._dev) if fill is None else torch.full(shape, fill, dtype=dtype, device=self._dev)
        t = torch.as_tensor(t, dtype=dtype, device=self._dev).contiguous()
        if tuple(t.shape) != shape:
            raise ValueError(f"{name} must have shape {shape}, got {tuple(t.shape)}")
        return t


class Progressive(_Frame):
    """A frame rendered a few samples at a time (DeviceScene.render_rows_range), bit-exact to one render_rows call.

    Owns -- or adopts, to resume a checkpoint -- the [rows, h, 3] float32 fold `sums` and the count `done` of samples folded
    into it.  `step(n)` renders the next min(n, samples - done) samples and returns the (avg, rgb) preview of the first
    `done` samples; to checkpoint, copy `sums` and `done` away, and pass them back in to resume, in this process or another.  A checkpoint
    also carries `depth`, the scene's path depth when the frame began: pass it back in as depth=, and a scene under another depth
    refuses to resume it (a fold that mixes depths is no frame); so does step() once the scene's depth was changed under the frame.
    A cast frame has no paths: its `depth` is None and it ignores the scene's.  The scene's sky (DeviceScene.set_sky) is treated
    exactly like the depth: `sky` records it (None or (up, down)), a checkpoint passes it back in as sky=, and a scene under
    another sky refuses to resume or to step.
    """

    def __init__(self, dscene, cam, samples, w, h, cast=False, shard=(None, 0, 1), sums=None, done=0, depth=None, sky=SCENE_SKY):
        samples, done = int(samples), int(done)
        if samples < 1:
            raise ValueError(f"samples must be positive, got {samples}")
        if not 0 <= done <= samples:
            raise ValueError(f"done must be in [0, {samples}], got {done}")
        rows = self._begin(dscene, cam, samples, w, h, cast, shard, depth=depth, sky=sky)
        if sums is None and done:
            raise ValueError("resuming (done > 0) needs the sums of the first `done` samples")
        self._sums, self._done = self._adopt("sums", sums, (rows, h, 3), torch.float32), done

    @property
    def sums(self):
        """The per-pixel fold over the first `done` samples (float32 CUDA tensor [rows, h, 3])."""
        return self._sums

    @property
    def done(self):
        """Samples folded into `sums` so far."""
        return self._done

    @property
    def finished(self):
        return self._done >= self.samples

    def step(self, n, stream=None):
        """Enqueue the next min(n, samples - done) samples; returns the (avg, rgb) CUDA tensors of the first `done` samples."""
        if self.finished:
            raise RuntimeError(f"the frame is finished: all {self.samples} samples are rendered")
        if int(n) < 1:
            raise ValueError(f"a step renders at least one sample, got {n}")
        self._unchanged()
        k_end = min(self._done + int(n), self.samples)
        avg, rgb = self.dscene.render_rows_range(self.cam, self.samples, self.w, self.h, self._done, k_end, self._sums,
                                                 cast=self.cast, shard=self.shard, stream=stream)
        self._done = k_end
        return avg, rgb


def rule_reference(sums, sums2, counts, mask, tol, eps):
    """The stopping rule of sq_adaptive_update_device restated in numpy float32, operation for operation: returns the new
    mask (uint8) of host arrays sums, sums2 [..., 3], counts, mask [...].  What the tests hold the kernel to."""
    import numpy as np
    f = np.float32
    with np.errstate(all="ignore"):
        s, q = np.asarray(sums, f), np.asarray(sums2, f)
        c = np.asarray(counts, np.int32)
        n = c.astype(f)
        ss = s * s
        lhs = n[..., None] * q - ss
        rhs = ss + f(eps) * (n * n)[..., None]
        L = (lhs[..., 0] + lhs[..., 1]) + lhs[..., 2]
        R = (rhs[..., 0] + rhs[..., 1]) + rhs[..., 2]
        converged = (c >= 2) & (L <= ((n - f(1)) * (f(tol) * f(tol))) * R)
    return ((np.asarray(mask) != 0) & ~converged).astype(np.uint8)


class _AdaptiveFrame(_Frame):
    """What Adaptive and AdaptiveLens share: the four state tensors and their adoption from a checkpoint, the picture, the live
    count under the gap guard, and a step's frame around the subclass's render call and built-in rule.  A subclass counts in a
    unit of its own (`_unit`: samples; sub-rays) of which the frame has `_limit`, each worth `_per` samples."""

    def _setup(self, dscene, cam, samples, w, h, cast, shard, limit, per, tol, eps, first, step, done, rule, state, depth, sky):
        """state: the constructor's sums, sums2, counts and mask by name.  Refuses in the constructors' one order."""
        done, first, step = int(done), int(first), int(step)
        tol, eps = float(tol), float(eps)
        if samples < 1:
            raise ValueError(f"samples must be positive, got {samples}")
        if not tol >= 0 or not eps >= 0:
            raise ValueError(f"tol and eps must be numbers >= 0, got {tol}, {eps}")
        if first < 1 or step < 1:
            raise ValueError(f"first and step must be positive, got {first}, {step}")
        if not 0 <= done <= limit:
            raise ValueError(f"done must be in [0, {limit}], got {done}")
        if rule is not None and not callable(rule):
            raise ValueError("rule must be callable: (sums, sums2, counts, mask) -> mask")
        if done and any(state[name] is None for name in _STATE):
            raise ValueError("resuming (done > 0) needs sums, sums2, counts and mask as the checkpoint left them")
        rows = self._begin(dscene, cam, samples, w, h, cast, shard, depth=depth, sky=sky)
        for name, fill in (("sums", 0), ("sums2", 0), ("counts", 0), ("mask", 1)):
            setattr(self, "_" + name, self._adopt(name, state[name], (rows, h) + _STATE[name][0], _STATE[name][1], fill))
        self._limit, self._per = limit, per
        self.tol, self.eps, self.first, self.step_size, self.rule = tol, eps, first, step, rule
        self._done = done
        self._avg = torch.zeros((rows, h, 3), dtype=torch.float32, device=self._dev)
        self._rgb = torch.zeros((rows, h, 3), dtype=torch.uint8, device=self._dev)
        if done:
            self._restore_picture()
        self._live = self._count_live()

    def _count_live(self):
        live = self._mask != 0
        if self._done:
            live &= self._counts == self._done           # a pixel left behind cannot resume (the gap guard of the masked call)
        return int(live.sum().item())

    def _restore_picture(self):
        """avg and rgb of a checkpoint: (1 / (float)(count * per)) *^ sum, as the call that last rendered the pixel wrote it
        (numpy's float32 division and product are the device's correctly rounded ones), and the device's own tonemap of it."""
        import numpy as np
        c = self._counts.cpu().numpy().astype(np.int64) * self._per
        s =self._sums.cpu().numpy()
        with np.errstate(all="ignore"):
            avg = (np.float32(1) / np.maximum(c, 1).astype(np.float32))[..., None] * s
        avg[c == 0] = 0
        rgb = N.debug_eval("tonemap", avg.reshape(-1, 3), device=self.dscene.device).reshape(avg.shape)
        rgb[c == 0] = 0
        self._avg.copy_(torch.from_numpy(np.ascontiguousarray(avg)))
        self._rgb.copy_(torch.from_numpy(np.ascontiguousarray(rgb)))

    sums = property(lambda self: self._sums, doc="Per-pixel fold of the radiances (of samples; of sub-ray sums) over the pixel's first counts units.")
    sums2 = property(lambda self: self._sums2, doc="Per-pixel fold of their squares over the same units.")
    counts = property(lambda self: self._counts, doc="Units (samples; sub-rays) each pixel has received (int32 CUDA tensor [rows, h]).")
    mask = property(lambda self: self._mask, doc="1 = the pixel is still live (uint8 CUDA tensor [rows, h]).")
    done = property(lambda self: self._done, doc="End of the last range (of samples; of sub-rays) rendered.")
    live = property(lambda self: self._live, doc="Pixels the next step would render.")

    @property
    def finished(self):
        return self._live == 0 or self._done >= self._limit

    @property
    def samples_spent(self):
        """Samples rendered so far, over all pixels (waits for the device)."""
        return int(self._counts.sum(dtype=torch.int64).item()) * self._per

    def step(self, stream=None):
        """Render the next range for the live pixels and apply the rule; returns the (avg, rgb) CUDA tensors of the frame."""
        if self.finished:
            raise RuntimeError("the frame is finished: no pixel is live" if self._live == 0
                               else f"the frame is finished: all {self._limit} {self._unit} are rendered")
        self._unchanged()
        end = min(self._done + (self.first if self._done == 0 else self.step_size), self._limit)
        self._render(self._done, end, stream)
        self._done = end
        if self.rule is None:
            self._builtin_rule(stream)
        else:
            self._callers_rule(stream)
        return self._avg, self._rgb

    def _callers_rule(self, stream):
        _, st = P.call_stream(self._mask.device, stream)
        with torch.cuda.stream(st):
            new = torch.as_tensor(self.rule(self._sums, self._sums2, self._counts, self._mask), device=self._mask.device)
            if tuple(new.shape) != tuple(self._mask.shape):
                raise ValueError(f"rule must return a mask of shape {tuple(self._mask.shape)}, got {tuple(new.shape)}")
            self._mask.copy_((new != 0).to(torch.uint8))
            self._live = self._count_live()


class Adaptive(_AdaptiveFrame):
    """A frame whose pixels stop receiving samples once a stopping rule calls them done (DeviceScene.render_rows_masked).

    Owns -- or adopts, to resume a checkpoint -- the folds `sums` and `sums2` [rows, h, 3], the per-pixel sample `counts` and
    the `mask` of live pixels [rows, h], and `done`, the end of the last range rendered.  `step()` renders the next range
    (`first` samples, then `step` at a time) for the live pixels, applies the rule and returns the (avg, rgb) picture, in
    which a pixel that stopped after n samples keeps the mean of its first n samples: bit for bit the reference's fold over
    the first n samples of the `samples`-sample frame.  rule: a callable (sums, sums2, counts, mask) -> new mask instead of
    the built-in rule (DeviceScene.adaptive_update with tol, eps), which is a heuristic -- a pixel that has seen nothing but
    black after `first` samples stops.  A pixel the rule switches back on after it was left out of a range stays out: its
    fold would have a gap.  To checkpoint, copy the four tensors, `done` and `depth` away and pass them back in (depth as in
    Progressive: a scene under another path depth refuses to resume), and `sky` likewise as sky=.
    """
    _unit = "samples"

    def __init__(self, dscene, cam, samples, w, h, tol, eps=1.0, first=8, step=8, cast=False, shard=(None, 0, 1), rule=None,
                 sums=None, sums2=None, counts=None, mask=None, done=0, depth=None, sky=SCENE_SKY):
        samples = int(samples)
        self._setup(dscene, cam, samples, w, h, cast, shard, samples, 1, tol, eps, first, step, done, rule,
                    dict(sums=sums, sums2=sums2, counts=counts, mask=mask), depth, sky)

    def _render(self, k_begin, k_end, stream):
        self.dscene.render_rows_masked(self.cam, self.samples, self.w, self.h, k_begin, k_end, self._sums, mask=self._mask,
                                       sums2=self._sums2, counts=self._counts, cast=self.cast, shard=self.shard, stream=stream,
                                       out_avg=self._avg, out_rgb=self._rgb)

    def _builtin_rule(self, stream):
        self._live = self.dscene.adaptive_update(self._sums, self._sums2, self._counts, self._mask, self.tol, self.eps, stream=stream)


NO_MOTION_RECORD = object()     # checkpoint_motion= of AdaptiveLens: a fresh frame, or a checkpoint that is trusted to match


def _motion_bits(motion):
    """A motion as bytes, so that two motions are the same when their bits are; None = a static camera."""
    return None if motion is None else motion.key()


def _motion_words(motion):
    return "no motion" if motion is None else f"the motion {motion!r}"


class AdaptiveLens(_AdaptiveFrame):
    """Adaptive for an anti-aliased, depth-of-field frame (DeviceScene.live_pixels, render_lens_masked): a pixel stops receiving
    SUB-RAYS once the stopping rule calls it done, and a stopped pixel costs no ray.

    The frame has `samples` samples and `subrays` sub-rays per pixel under `lens` (lens.py), n = samples / subrays samples on each
    sub-ray.  Everything Adaptive counts in samples is counted in sub-rays here: `first` and `step`, `done`, and `counts` -- the
    terms of `sums2` are sub-ray sums, and the rule's n must be the number of terms.  `sample_counts` is counts * n.  `step()`
    lists the live pixels, renders their next sub-rays, applies the rule and returns the (avg, rgb) picture, in which a pixel that
    stopped after c sub-rays keeps (1 / (c * n)) * sum: bit for bit render_lens over r_range = (0, c).  rule: a callable (sums,
    sums2, counts, mask) -> new mask instead of the built-in one, which is DeviceScene.adaptive_update with tol and eps * n * n:
    the sub-ray sums are n times a sample's size, so that is Adaptive's criterion on the pixel mean.  The gap guard, checkpoints,
    depth= and sky= are Adaptive's.  work_mb: as in render_lens.

    motion (a Motion; None = the frame as it was, under `cam`): the frame is motion-blurred -- every step goes through
    render_shutter_masked and `cam` is not read.  The frame records the motion as it records depth and sky: `motion` is part of a
    checkpoint, to be passed back in, and a checkpoint (done > 0) resumed under another motion -- compared by bits -- or under none
    is refused with checkpoint_motion=, which is what the checkpoint carried (the default, NO_MOTION_RECORD, is a fresh frame)."""
    _unit = "sub-rays"

    def __init__(self, dscene, cam, lens, samples, subrays, w, h, tol, eps=1.0, first=1, step=1, shard=(None, 0, 1), rule=None,
                 sums=None, sums2=None, counts=None, mask=None, done=0, depth=None, sky=SCENE_SKY, work_mb=None, motion=None,
                 checkpoint_motion=NO_MOTION_RECORD):
        from .lens import frame_args
        samples, subrays, _, _ = frame_args(lens, samples, subrays)
        if motion is not None:
            from .shutter import motion_arg
            motion_arg(motion)
        if checkpoint_motion is not NO_MOTION_RECORD and _motion_bits(checkpoint_motion) != _motion_bits(motion):
            raise N.SquiglyError(f"the checkpoint was rendered under {_motion_words(checkpoint_motion)}, the frame is given "
                                 f"{_motion_words(motion)}: pass the checkpoint's motion as motion=")
        self.motion = motion
        self.lens, self.subrays, self.n, self.work_mb = lens, subrays, samples // subrays, work_mb
        self._setup(dscene, cam, samples, w, h, False, shard, subrays, self.n, tol, eps, first, step, done, rule,
                    dict(sums=sums, sums2=sums2, counts=counts, mask=mask), depth, sky)

    sample_counts = property(lambda self: self._counts * self.n, doc="Samples each pixel has received: counts * n.")

    def _render(self, r_begin, r_end, stream):
        index, _ = self.dscene.live_pixels(self._mask, self._counts, r_begin, stream=stream)
        # the list's length is the live count the last step (or the constructor) already brought to the host: no wait here
        if self.motion is not None:
            self.dscene.render_shutter_masked(self.motion, self.lens, self.samples, self.subrays, self.w, self.h, r_begin, r_end,
                                              self._sums, index, self._live, sums2=self._sums2, counts=self._counts, shard=self.shard,
                                              work_mb=self.work_mb, out_avg=self._avg, out_rgb=self._rgb, stream=stream)
            return
        self.dscene.render_lens_masked(self.cam, self.lens, self.samples, self.subrays, self.w, self.h, r_begin, r_end, self._sums,
                                       index, self._live, sums2=self._sums2, counts=self._counts, shard=self.shard,
                                       work_mb=self.work_mb, out_avg=self._avg, out_rgb=self._rgb, stream=stream)

    def _builtin_rule(self, stream):
        self.dscene.adaptive_update(self._sums, self._sums2, self._counts, self._mask, self.tol, self.eps * self.n * self.n, stream=stream)
        # the next list's length is the gap-guarded count, which is the rule's own unless a checkpoint brought a pixel with a gap
        _, st = P.call_stream(self._mask.device, stream)
        with torch.cuda.stream(st):
            self._live = self._count_live()
