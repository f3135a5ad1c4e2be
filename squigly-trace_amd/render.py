"""Mirror of the reference's `Lib` module (src/Lib.hs): Settings and render.

    render :: Scene a -> Camera -> Settings -> IO ()          src/Lib.hs:68-75
Here `render(bih, cam, settings)` fills the same w-rows x h-columns RGB8 image through
sq_render_rgb8 — the foreign call that replaces src/Lib.hs:73-74 — and writes the PNG.
"""
import contextlib
import ctypes as C
from dataclasses import dataclass, field
from typing import Tuple

import numpy as np

from . import _native as N
from .png import write_png


@dataclass
class Settings:
    """src/Lib.hs:54-63, defaults from app/Main.hs:13-30."""
    samples: int = 10
    dimensions: Tuple[int, int] = (540, 540)
    savePath: str = "./render/result.png"
    objPath: str = "./data/scene.obj"
    cameraPath: str = "./data/camera"
    debug: bool = False
    debugPath: str = ""
    cast: bool = False


def render_rgb8(bih, cam, samples, dimensions, cast=False) -> np.ndarray:
    """The array `img` of src/Lib.hs:74: shape (w, h, 3) uint8 — w ROWS, h COLUMNS."""
    w, h = dimensions
    out = np.empty((max(w, 0), max(h, 0), 3), np.uint8)
    N.check(N.lib().sq_render_rgb8(C.byref(bih.scene), C.byref(cam), samples, w, h, int(bool(cast)), out.ctypes.data))
    return out


def render_f32(bih, cam, samples, dimensions, cast=False) -> np.ndarray:
    """The pre-tonemap `avg` of src/Lib.hs:88 for every pixel: shape (w, h, 3) float32."""
    w, h = dimensions
    out = np.empty((max(w, 0), max(h, 0), 3), np.float32)
    N.check(N.lib().sq_render_f32(C.byref(bih.scene), C.byref(cam), samples, w, h, int(bool(cast)), out.ctypes.data))
    return out


def _resident(bih, device, lights, depth, sky):
    """What the resident-scene wrappers share.  The call itself refuses a depth or a sky that is not one, before anything is
    uploaded; the context manager it returns uploads the scene on entry (DeviceScene), sets those of lights, depth and sky that
    are not None, and closes the scene on exit."""
    if depth is not None:
        N.depth_value(depth)
    sky = N.sky_pair(sky)

    @contextlib.contextmanager
    def scene():
        from .device import DeviceScene                # torch: only the resident-scene path needs it
        ds = DeviceScene(bih, device)
        try:
            if lights is not None:
                ds.set_lights(lights)
            if depth is not None:
                ds.set_depth(depth)
            if sky is not None:
                ds.set_sky(sky[0], sky[1])
            yield ds
        finally:
            ds.close()
    return scene()


def render_progressive(bih, cam, samples, dimensions, step, cast=False, device=0, lights=None, depth=None, sky=None):
    """The frame of render_rgb8, `step` samples at a time: yields (done, rgb8) after every step, rgb8 being the (w, h, 3) uint8
    image of the first `done` samples.  The last image (done == samples) is bit for bit that of render_rgb8 (DeviceScene,
    Progressive: one device, the scene uploaded once).  lights: the point lights of a cast frame (DeviceScene.set_lights; None = the
    reference's light).  depth: the path depth of a path-traced frame (DeviceScene.set_depth; None = the reference's 3, which is
    what render_rgb8 computes); a depth is refused before anything is uploaded when it is not an integer in 1..8.  sky: the sky of a
    path-traced frame (DeviceScene.set_sky): three numbers (a constant sky) or (up, down); None = no sky, the reference's black.
    Refused before anything is uploaded when it is neither."""
    from .device import Progressive                    # torch: only the resident-scene path needs it
    w, h = dimensions
    if int(step) < 1:
        raise ValueError(f"step must be positive, got {step}")
    with _resident(bih, device, lights, depth, sky) as ds:
        p = Progressive(ds, cam, samples, w, h, cast=cast)
        while not p.finished:
            _, rgb = p.step(step)
            yield p.done, rgb.cpu().numpy()


def denoise_options(denoise):
    """denoise= of render_adaptive as keyword arguments of denoise_frame: True = the defaults, a number = sigma_l, a dict = itself."""
    if denoise is True:
        return {}
    if isinstance(denoise, dict):
        return dict(denoise)
    if isinstance(denoise, (int, float)) and not isinstance(denoise, bool) and float(denoise) > 0:
        return {"sigma_l": float(denoise)}
    raise ValueError(f"denoise must be True, a sigma_l > 0 or a dict of denoise parameters, got {denoise!r}")


def denoise_arg(denoise):
    """denoise= of render_adaptive, render_sequence and Temporal: None (None or False: off), or denoise_options of it."""
    return None if denoise is None or denoise is False else denoise_options(denoise)


def render_adaptive(bih, cam, samples, dimensions, tol, eps=1.0, first=8, step=8, cast=False, device=0, rule=None, lights=None,
                    depth=None, sky=None, denoise=None, lens=None, subrays=None, motion=None, film=None):
    """The frame of render_rgb8 with adaptive sampling (DeviceScene, Adaptive): yields (done, live, spent, rgb8, counts) after
    every step -- the end of the range rendered, the pixels still live, the samples spent so far, the (w, h, 3) uint8 image and
    the (w, h) int32 per-pixel sample counts.  A pixel that stopped after n samples shows the mean of its first n samples, so
    with first >= samples (one step, every pixel live) the image is bit for bit that of render_rgb8.  lights, depth, sky: as in
    render_progressive.  denoise (None = off; True, a sigma_l or a dict of denoise parameters): once the frame is finished, one more
    tuple follows whose image is the frame filtered on the device (denoise_frame: the variance from the frame's own second moments,
    the guides from its first hits) and tonemapped by the device's own tonemap; the tuples before it are unchanged.
    lens (a Lens; None = no lens, the function as it was) and subrays (None = samples): the anti-aliased, depth-of-field frame of
    render_lens_rgb8, adaptively sampled in whole sub-rays (AdaptiveLens).  first and step stay in samples and must be multiples of
    n = samples / subrays (ValueError); the yielded done, spent and counts are samples too; cast=True is refused.  denoise= then
    filters with the variance of the sub-ray sums brought to the pixel mean's scale, denoise_variance(...) * (1 / (n * n)).
    motion (a Motion; needs a lens): the lens frame under a camera that moves during the exposure (AdaptiveLens(motion=)); cam is then
    not read, and denoise= takes its guides from motion.pose(0.5) -- a convenience, not pinned to the bit.
    film (a Film; needs denoise): the last tuple's image is developed by it on the device (libsquigly_film.so) and leaves the device
    only as bytes; None = the device's own tonemap through the debug hook, as before.  Film() gives the same bytes."""
    from .device import Adaptive, AdaptiveLens         # torch: only the resident-scene path needs it
    from .film import film_arg
    w, h = dimensions
    if film_arg(film) is not None and (denoise is None or denoise is False):
        raise ValueError("film needs denoise: only the filtered frame is developed (the steps before it are the renderer's own bytes)")
    if int(first) < 1 or int(step) < 1:
        raise ValueError(f"first and step must be positive, got {first}, {step}")
    if not float(tol) >= 0 or not float(eps) >= 0:
        raise ValueError(f"tol and eps must be numbers >= 0, got {tol}, {eps}")
    n = None                                           # samples on a sub-ray: an AdaptiveLens counts in sub-rays, the caller in samples
    if lens is not None or subrays is not None or motion is not None:
        from .lens import frame_args
        if lens is None:
            raise ValueError("subrays and motion need a lens")
        if motion is not None:
            from .shutter import motion_arg
            motion_arg(motion)
        if cast:
            raise ValueError("a lens frame is path-traced: cast=True is refused")
        S, R, _, _ = frame_args(lens, samples, samples if subrays is None else subrays)
        n = S // R
        if int(first) % n or int(step) % n:
            raise ValueError(f"first and step must be multiples of samples / subrays = {n}, got {first}, {step}")
    scene = _resident(bih, device, lights, depth, sky)
    dn = denoise_arg(denoise)                          # refused before anything is uploaded
    with scene as ds:
        if n is None:
            a = Adaptive(ds, cam, samples, w, h, tol, eps=eps, first=first, step=step, cast=cast, rule=rule)
            done, counts = (lambda: a.done), (lambda: a.counts)
        else:
            a = AdaptiveLens(ds, cam, lens, S, R, w, h, tol, eps=eps, first=int(first) // n, step=int(step) // n, rule=rule, motion=motion)
            done, counts = (lambda: a.done * n), (lambda: a.sample_counts)
        avg = None
        while not a.finished:
            avg, rgb = a.step()
            yield done(), a.live, a.samples_spent, rgb.cpu().numpy(), counts().cpu().numpy()
        if dn is not None and avg is not None:       # (a frame without pixels never steps: nothing to filter)
            from .denoise import denoise_frame, denoise_variance
            var = denoise_variance(a.sums, a.sums2, a.counts)
            if n is not None:
                # the variance of the mean of sub-ray sums is n * n times that of the pixel mean, in every branch of the variance formula
                var = var * (1 / (n * n))                                                    # one float32 multiply
            out, _ = denoise_frame(ds, cam if motion is None else motion.pose(0.5), w, h, avg, var=var, **dn)
            img = _developed(ds, out, film)
            yield done(), a.live, a.samples_spent, img, counts().cpu().numpy()


def _developed(ds, out, film):
    """The uint8 image of a filtered device frame: film's, which leaves the device as bytes only, or -- film None -- the device's
    own tonemap through the debug hook (a host round trip of the float frame)."""
    if film is not None:
        return film(out).cpu().numpy()
    return N.debug_eval("tonemap", out.cpu().numpy().reshape(-1, 3), device=ds.device).reshape(tuple(out.shape))


def render_views_rgb8(bih, cams, samples, dimensions, cast=False, device=0, lights=None, depth=None, sky=None) -> np.ndarray:
    """The image of render_rgb8 for every camera of `cams`, rendered in one call (DeviceScene.render_views): shape (n, w, h, 3)
    uint8, view i bit for bit render_rgb8 of cams[i].  lights, depth, sky: as in render_progressive (every view has the same lights, depth
    and sky)."""
    cams = list(cams)
    if not cams:
        raise ValueError("render_views_rgb8 needs at least one camera")
    scene = _resident(bih, device, lights, depth, sky)
    import torch
    w, h = dimensions
    with scene as ds:
        _, rgb = ds.render_views(cams, samples, w, h, cast=cast, want_avg=False)
        torch.cuda.synchronize(ds.device)
        return rgb.cpu().numpy()


def render_lens_rgb8(bih, cam, samples, dimensions, lens=None, subrays=None, device=0, depth=None, sky=None, work_mb=None,
                     motion=None) -> np.ndarray:
    """The image of render_rgb8 with anti-aliasing and depth of field (DeviceScene.render_lens): shape (w, h, 3) uint8.  lens: a
    Lens (None = Lens(): a box filter over the pixel, no aperture).  subrays: primary rays per pixel, a divisor of samples (None =
    samples, a ray per sample).  With Lens(jitter=0) and subrays=1 the image is bit for bit that of render_rgb8.  depth, sky: as in
    render_progressive.  motion (a Motion): the frame under a camera that moves during the exposure (DeviceScene.render_shutter); cam
    is then not read.  Refused before anything is uploaded: what lens.frame_args and shutter.motion_arg refuse."""
    from .lens import Lens, frame_args
    lens = Lens() if lens is None else lens
    subrays = samples if subrays is None else subrays
    frame_args(lens, samples, subrays)
    if motion is not None:
        from .shutter import motion_arg
        motion_arg(motion)
    scene = _resident(bih, device, None, depth, sky)
    import torch
    w, h = dimensions
    with scene as ds:
        if motion is None:
            out = ds.render_lens(cam, lens, samples, subrays, w, h, want_avg=False, work_mb=work_mb)
        else:
            out = ds.render_shutter(motion, lens, samples, subrays, w, h, want_avg=False, work_mb=work_mb)
        torch.cuda.synchronize(ds.device)
        return out.rgb.cpu().numpy()


def render_sequence(bih, cams, spp, dimensions, temporal=True, denoise=None, device=0, depth=None, sky=None, period=64, alpha_min=0.1,
                    max_history=32, film=None, sparse=None, clamp=None):
    """The frames of a camera move, `spp` samples each (DeviceScene, Temporal: one device, the scene uploaded once): yields the
    (w, h, 3) uint8 image of every camera of `cams`, in order.  temporal=True accumulates every frame over the ones before it
    (libsquigly_temporal.so); temporal=False shows each frame's own samples -- the same samples, so the two can be compared.
    Frame f takes the samples [(f mod period) * spp, + spp) of the (spp * period)-sample frame.  denoise (None = off; True, a
    sigma_l or a dict of denoise parameters): every frame is filtered on the device after the accumulation.  depth, sky: as in
    render_progressive.  The images are a preview's (temporal.tonemap), not pinned to the bit, unless film (a Film) is given: every
    frame is then developed by it on the device (libsquigly_film.so; with Film(auto=...) the exposure adapts from frame to frame under
    temporal=True; under temporal=False the film's exposure state is forgotten after every frame as the history is -- film.reset() --
    so that every frame is exposed at its own target and the frames stay independent).
    sparse (None = off; a stride S in 1..16): every frame traces only a lattice of its pixels, which moves from frame to frame, and
    the holes, and fills the others in from their traced neighbours (Temporal(sparse=S)).  clamp: Temporal's (None = off).
    Refused before anything is uploaded: no camera, what Temporal refuses of spp, period, alpha_min and max_history, and a sparse
    that is no stride."""
    cams = list(cams)
    if not cams:
        raise ValueError("render_sequence needs at least one camera")
    from .temporal import _temporal_args
    _temporal_args(spp, period, alpha_min, max_history)
    from .temporal import clamp_arg
    clamp_arg(clamp)
    if sparse is not None:
        from .denoise import stride_arg
        stride_arg(sparse)
    from .film import film_arg
    film_arg(film)
    dn = denoise_arg(denoise)                          # refused before anything is uploaded
    scene = _resident(bih, device, None, depth, sky)
    w, h = dimensions
    with scene as ds:
        from .temporal import Temporal                 # torch: only the resident-scene path needs it
        t = Temporal(ds, w, h, spp, period=period, alpha_min=alpha_min, max_history=max_history, denoise=dn, film=film, sparse=sparse,
                     clamp=clamp)
        for cam in cams:
            _, _, _, rgb = t.step(cam)
            if not temporal:
                t.forget()
                if film is not None:
                    film.reset()
            yield rgb.cpu().numpy()


MOVING_BUILD_DEVICE_FROM = 50000     # triangles from which a frame's tree is built on the device (DESIGN.md 4.28's measurement)


def render_moving_sequence(mesh, cams, poses, spp, dimensions, temporal=True, clamp=None, denoise=None, device=0, depth=None, sky=None,
                           period=64, alpha_min=0.1, max_history=32, film=None, build=None):
    """render_sequence under geometry that moves rigidly: `mesh` is the scene in its rest pose and poses [frames, n_materials, 3, 4]
    gives every material's pose [R | t] (world = R local + t) in every frame -- the objects are the materials.  Per frame the mesh
    is moved (moved_mesh), its tree built, the scene uploaded (a DeviceScene per frame: nothing is refitted in place) and stepped
    with the move from the frame before (Temporal.step(cam, scene=, back=back_transforms(...))).  Yields the (w, h, 3) uint8 image
    of every frame.  clamp: Temporal's (None = off).  build: "host" or "device", where a frame's tree is built; None = on the device
    from MOVING_BUILD_DEVICE_FROM triangles up.  temporal=False shows each frame's own samples.
    Refused before anything is uploaded: no camera, poses that are not a [len(cams), n_materials, 3, 4] array, what Temporal
    refuses of its numbers, a build that is neither."""
    from .scene import BIH, moved_mesh
    cams = list(cams)
    if not cams:
        raise ValueError("render_moving_sequence needs at least one camera")
    poses = np.asarray(poses, np.float64)
    if poses.shape != (len(cams), len(mesh.materials), 3, 4):
        raise ValueError(f"poses must have shape ({len(cams)}, {len(mesh.materials)}, 3, 4): a pose per frame and material, got {poses.shape}")
    if build not in (None, "host", "device"):
        raise ValueError(f"build must be 'host', 'device' or None, got {build!r}")
    from .temporal import _temporal_args, back_transforms, clamp_arg
    _temporal_args(spp, period, alpha_min, max_history)
    clamp_arg(clamp)
    from .film import film_arg
    film_arg(film)
    dn = denoise_arg(denoise)
    on_device = build == "device" or (build is None and len(mesh) >= MOVING_BUILD_DEVICE_FROM)
    w, h = dimensions
    t = None
    for f, cam in enumerate(cams):
        bih = BIH(moved_mesh(mesh, poses[f]), device=device if on_device else None)
        with _resident(bih, device, None, depth, sky) as ds:
            if t is None:
                from .temporal import Temporal
                t = Temporal(ds, w, h, spp, period=period, alpha_min=alpha_min, max_history=max_history, denoise=dn, film=film, clamp=clamp)
            _, _, _, rgb = t.step(cam, scene=ds, back=None if f == 0 else back_transforms(poses[f - 1], poses[f]))
            if not temporal:
                t.forget()
                if film is not None:
                    film.reset()
            img = rgb.cpu().numpy()                  # (waits for the frame: its scene may close)
        yield img


def render_sparse(bih, cam, samples, dimensions, stride, offset=(0, 0), denoise=None, film=None, device=0, depth=None, sky=None,
                  sigma_p=None, cos_n=0.9, demodulate=True) -> np.ndarray:
    """The frame of render_rgb8 traced sparsely: only the pixels of the lattice of `stride` and `offset` = (oy, ox), and the holes
    between them, are traced (denoise.sparse_mask, DeviceScene.render_rows_masked); every other pixel is filled in from its traced
    neighbours on the same surface (denoise.upsample), in demodulated space unless demodulate=False.  Shape (w, h, 3) uint8.  A
    traced pixel holds the dense frame's average bit for bit; with stride 1 the whole frame does.  sigma_p (None =
    denoise.default_sigma_p of the scene) and cos_n are the stops of a neighbour.  denoise (None = off; True, a sigma_l or a dict of
    denoise parameters) filters the filled-in frame with the variance of its own second moments; film (a Film) develops it on the
    device, None = the device's own tonemap.  depth, sky: as in render_progressive.  Path-traced frames, whole, on one device.
    Refused before anything is uploaded: a stride outside 1..16, an offset outside [0, stride), samples < 1."""
    from .denoise import lattice_args
    from .film import film_arg
    lattice_args(stride, offset)
    if isinstance(samples, bool) or int(samples) < 1:
        raise ValueError(f"samples must be a positive integer, got {samples!r}")
    film = film_arg(film)
    dn = denoise_arg(denoise)
    scene = _resident(bih, device, None, depth, sky)
    w, h = dimensions
    with scene as ds:
        import importlib
        import torch
        D = importlib.import_module(__package__ + ".denoise")           # (the package's own `denoise` is the function)
        sp = D.default_sigma_p(ds.bih.bounds) if sigma_p is None else float(sigma_p)
        if dn is not None:
            dn.setdefault("sigma_p", sp)
            D.make_params(**dn)
        lattice = dict(stride=stride, offset=offset, sigma_p=sp, cos_n=cos_n)
        dev = torch.device("cuda", ds.device)
        g = ds.guides(cam, w, h)
        live = D.sparse_mask(g, **lattice)
        rows = int(live.shape[0])
        sums = torch.zeros((rows, h, 3), dtype=torch.float32, device=dev)
        sums2 = torch.zeros_like(sums) if dn is not None else None
        avg, _ = ds.render_rows_masked(cam, samples, w, h, 0, samples, sums, mask=live, sums2=sums2, want_rgb=False)
        var = None
        if dn is not None:
            var = D.denoise_variance(sums, sums2, torch.full((rows, h), int(samples), dtype=torch.int32, device=dev))
        x, how = avg, None
        if demodulate:
            x, var, how = D.demodulated(g, avg, var)
        out, out_var = D.upsample(x, g, live, var=var, **lattice)
        if dn is not None:
            out, out_var = D.denoise(out, g.tri, g.normal, g.point, var=out_var, **dn)
        if how is not None:
            out, _ = D.remodulated(g, out, out_var, how)
        return _developed(ds, out, film)


def render(bih, cam, settings: Settings):
    """Lib.render: compute the image and write it to settings.savePath."""
    img = render_rgb8(bih, cam, settings.samples, settings.dimensions, settings.cast)
    write_png(settings.savePath, img)
    return img
