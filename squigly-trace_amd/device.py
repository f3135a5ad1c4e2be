"""Resident-scene rendering on one MI355X: the scene is uploaded once, frames stay in HBM.

PyTorch is used only for device memory and streams (plumbing); every pixel is produced by the HIP
kernels in csrc/sq_device.hip through the C-ABI of include/squigly_hip.h.
"""
import collections
import ctypes as C

import torch

from . import _native as N

Hits = collections.namedtuple("Hits", ["tri", "dist", "point"])
Hits.__doc__ = """Results of DeviceScene.intersect: Maybe Intersection (src/Geometry.hs:71-75) per ray; tri = -1 is Nothing."""


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


class DeviceScene:
    """A BIH uploaded to one GPU (sq_scene_upload)."""

    def __init__(self, bih, device=0):
        self.bih = bih                      # keeps the host arrays alive
        self.device = int(device)
        h = C.c_void_p()
        N.check(N.lib().sq_scene_upload(C.byref(bih.scene), self.device, C.byref(h)))
        self._h = h

    def set_option(self, key, value):
        N.check(N.lib().sq_set_option(self._h, key.encode(), int(value)))

    def _outputs(self, w, h, shard, want_avg, want_rgb, stream, out_avg, out_rgb, views=None):
        """(sq_shard, rows, out_avg, out_rgb, stream) of a render_rows* call: the shard's row count, the output tensors
        (allocated unless given or not wanted) and the stream (default: the device's current one).  views: the tensors get a
        leading dimension of that many views (render_views)."""
        rb, si, ns = shard
        sh = N.Shard(int(w if rb is None else rb), int(si), int(ns))
        rows = N.lib().sq_shard_rows(w, sh)
        if rows < 0:
            raise N.SquiglyError(f"bad shard {shard}")
        dev = torch.device("cuda", self.device)
        shape = (rows, h, 3) if views is None else (views, rows, h, 3)
        if want_avg and out_avg is None:
            out_avg = torch.empty(shape, dtype=torch.float32, device=dev)
        if want_rgb and out_rgb is None:
            out_rgb = torch.empty(shape, dtype=torch.uint8, device=dev)
        st = stream if stream is not None else torch.cuda.current_stream(dev)
        return sh, rows, out_avg, out_rgb, st

    def render_rows(self, cam, samples, w, h, cast=False, shard=(None, 0, 1), want_avg=True, want_rgb=True,
                    stream=None, out_avg=None, out_rgb=None):
        """Enqueue the render of this shard's rows; returns (avg, rgb) CUDA tensors [rows, h, 3].

        shard = (row_block, shard_index, n_shards); row_block None = all rows in one block.
        """
        sh, _, out_avg, out_rgb, st = self._outputs(w, h, shard, want_avg, want_rgb, stream, out_avg, out_rgb)
        N.check(N.lib().sq_render_rows_device(
            self._h, C.byref(cam), samples, w, h, int(bool(cast)), sh,
            out_avg.data_ptr() if out_avg is not None else None,
            out_rgb.data_ptr() if out_rgb is not None else None,
            C.c_void_p(st.cuda_stream)))
        return out_avg, out_rgb

    def render_rows_range(self, cam, samples, w, h, k_begin, k_end, sums, cast=False, shard=(None, 0, 1), want_avg=True,
                          want_rgb=True, stream=None, out_avg=None, out_rgb=None):
        """Enqueue the samples [k_begin, k_end) of the `samples`-sample frame (sq_render_rows_device_range); returns (avg, rgb)
        of the k_end samples folded so far.

        sums: float32 CUDA tensor [rows, h, 3] on this device, the per-pixel fold over [0, k_begin) on entry (ignored when
        k_begin == 0) and over [0, k_end) once the stream gets there.
        """
        sh, rows, out_avg, out_rgb, st = self._outputs(w, h, shard, want_avg, want_rgb, stream, out_avg, out_rgb)
        if sums is None:
            raise N.SquiglyError("render_rows_range needs a sums tensor")
        if (tuple(sums.shape) != (rows, h, 3) or sums.dtype != torch.float32 or not sums.is_contiguous()
                or sums.device != torch.device("cuda", self.device)):
            raise N.SquiglyError(f"sums must be a contiguous float32 tensor of shape {(rows, h, 3)} on cuda:{self.device}, "
                                 f"got {sums.dtype} {tuple(sums.shape)} on {sums.device}")
        N.check(N.lib().sq_render_rows_device_range(
            self._h, C.byref(cam), samples, w, h, int(bool(cast)), sh, int(k_begin), int(k_end), sums.data_ptr(),
            out_avg.data_ptr() if out_avg is not None else None,
            out_rgb.data_ptr() if out_rgb is not None else None,
            C.c_void_p(st.cuda_stream)))
        return out_avg, out_rgb

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
        sh, rows, out_avg, out_rgb, st = self._outputs(w, h, shard, want_avg, want_rgb, stream, out_avg, out_rgb, views=n)
        if sums is not None and (tuple(sums.shape) != (n, rows, h, 3) or sums.dtype != torch.float32 or not sums.is_contiguous()
                                 or sums.device != torch.device("cuda", self.device)):
            raise N.SquiglyError(f"sums must be a contiguous float32 tensor of shape {(n, rows, h, 3)} on cuda:{self.device}, "
                                 f"got {sums.dtype} {tuple(sums.shape)} on {sums.device}")
        table = (N.Camera * n)(*cams)
        N.check(N.lib().sq_render_views_device(
            self._h, table, n, samples, w, h, int(bool(cast)), sh, int(k_begin), k_end,
            sums.data_ptr() if sums is not None else None,
            out_avg.data_ptr() if out_avg is not None else None,
            out_rgb.data_ptr() if out_rgb is not None else None,
            C.c_void_p(st.cuda_stream)))
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
        dev = torch.device("cuda", self.device)
        st = stream if stream is not None else torch.cuda.current_stream(dev)
        lead = shape[:-1]
        out = Hits(*(out if out is not None else (None, None, None)))
        for name, t, want, tshape, dtype in (("tri", out.tri, True, lead, torch.int32), ("dist", out.dist, want_dist, lead, torch.float32),
                                             ("point", out.point, want_point, shape, torch.float32)):
            if t is not None and want and (tuple(t.shape) != tuple(tshape) or t.dtype != dtype or not t.is_contiguous() or t.device != dev):
                raise N.SquiglyError(f"out.{name} must be a contiguous {dtype} tensor of shape {tuple(tshape)} on {dev}, "
                                     f"got {t.dtype} {tuple(t.shape)} on {t.device}")
        with torch.cuda.stream(st):      # temporaries are allocated and freed in the order of the call's stream
            o = torch.as_tensor(origins, device=dev).to(torch.float32).contiguous()
            d = torch.as_tensor(directions, device=dev).to(torch.float32).contiguous()
            tri = out.tri if out.tri is not None else torch.empty(lead, dtype=torch.int32, device=dev)
            dist = (out.dist if out.dist is not None else torch.empty(lead, dtype=torch.float32, device=dev)) if want_dist else None
            point = (out.point if out.point is not None else torch.empty(shape, dtype=torch.float32, device=dev)) if want_point else None
            N.check(N.lib().sq_intersect_rays_device(
                self._h, o.data_ptr(), d.data_ptr(), int(o.numel() // 3), tri.data_ptr(),
                dist.data_ptr() if dist is not None else None, point.data_ptr() if point is not None else None,
                C.c_void_p(st.cuda_stream)))
        return Hits(tri, dist, point)

    def camera_rays(self, cam, w, h, shard=(None, 0, 1), stream=None):
        """The primary ray of every pixel of the shard, as the renderer traces it (sq_camera_rays_device): (origins,
        directions) float32 CUDA tensors [rows, h, 3].  ds.intersect(*ds.camera_rays(cam, w, h)) is the frame's depth and
        triangle-id buffer."""
        sh, rows, _, _, st = self._outputs(w, h, shard, False, False, stream, None, None)
        dev = torch.device("cuda", self.device)
        o = torch.empty((rows, h, 3), dtype=torch.float32, device=dev)
        d = torch.empty((rows, h, 3), dtype=torch.float32, device=dev)
        N.check(N.lib().sq_camera_rays_device(self._h, C.byref(cam), int(w), int(h), sh, o.data_ptr(), d.data_ptr(),
                                              C.c_void_p(st.cuda_stream)))
        return o, d

    def enable_timing(self, on=True):
        """Bracket every launch of the dominant kernel with hipEvents (read back by kernel_timing)."""
        self.set_option("timing", int(bool(on)))

    def kernel_timing(self):
        """(average ms per launch of the dominant kernel, launches, kernel name) since the last reset."""
        ms, n, name = C.c_double(), C.c_int64(), C.c_char_p()
        N.check(N.lib().sq_kernel_timing(self._h, C.byref(ms), C.byref(n), C.byref(name)))
        return ms.value, n.value, (name.value or b"").decode()

    def stats(self, reset=False):
        """Cumulative trace-kernel statistics: [rays traced, profile counters...] (synchronises)."""
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

    def close(self):
        if getattr(self, "_h", None) and N is not None and N._lib is not None:
            N._lib.sq_scene_free(self._h)
        self._h = None

    __del__ = close


class Progressive:
    """A frame rendered a few samples at a time (DeviceScene.render_rows_range), bit-exact to one render_rows call.

    Owns -- or adopts, to resume a checkpoint -- the [rows, h, 3] float32 fold `sums` and the count `done` of samples folded
    into it.  `step(n)` renders the next min(n, samples - done) samples and returns the (avg, rgb) preview of the first
    `done` samples; to checkpoint, copy `sums` and `done` away, and pass them back in to resume, in this process or another.
    """

    def __init__(self, dscene, cam, samples, w, h, cast=False, shard=(None, 0, 1), sums=None, done=0):
        samples, done = int(samples), int(done)
        if samples < 1:
            raise ValueError(f"samples must be positive, got {samples}")
        if not 0 <= done <= samples:
            raise ValueError(f"done must be in [0, {samples}], got {done}")
        rb, si, ns = shard
        rows = N.lib().sq_shard_rows(w, N.Shard(int(w if rb is None else rb), int(si), int(ns)))
        if rows < 0:
            raise N.SquiglyError(f"bad shard {shard}")
        dev = torch.device("cuda", dscene.device)
        if sums is None:
            if done:
                raise ValueError("resuming (done > 0) needs the sums of the first `done` samples")
            sums = torch.empty((rows, h, 3), dtype=torch.float32, device=dev)
        else:   # adopts a matching CUDA tensor as it is; anything else (a host copy) is copied to the device
            sums = torch.as_tensor(sums, dtype=torch.float32, device=dev).contiguous()
            if tuple(sums.shape) != (rows, h, 3):
                raise ValueError(f"sums must have shape {(rows, h, 3)}, got {tuple(sums.shape)}")
        self.dscene, self.cam, self.samples, self.w, self.h = dscene, cam, samples, int(w), int(h)
        self.cast, self.shard = bool(cast), shard
        self._sums, self._done = sums, done

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
        k_end = min(self._done + int(n), self.samples)
        avg, rgb = self.dscene.render_rows_range(self.cam, self.samples, self.w, self.h, self._done, k_end, self._sums,
                                                 cast=self.cast, shard=self.shard, stream=stream)
        self._done = k_end
        return avg, rgb
