"""squigly-trace on MI355X: the per-pixel sampling loop of rrruko/squigly-trace as HIP kernels.

Import with importlib (the directory name contains a hyphen):
    sqt = importlib.import_module("squigly-trace_amd")
"""
from ._native import Camera, Shard, SquiglyError, lib, LIB_PATH, EXPORTED_SYMBOLS, debug_eval, build_id, REFERENCE_LIGHT, MAX_LIGHTS  # noqa: F401
from .scene import BIH, Mesh, load_camera, camera_from_text, rot_matrix_rads, moved_mesh       # noqa: F401
from .render import Settings, render, render_rgb8, render_f32, render_progressive, render_adaptive, render_views_rgb8, render_lens_rgb8, render_sequence, render_sparse, render_moving_sequence   # noqa: F401
from .png import write_png                                                          # noqa: F401
# the filter: sqt.denoise is the function; its module is importlib.import_module("squigly-trace_amd.denoise")
from .denoise import denoise, denoise_variance, denoise_frame, Guides                # noqa: F401
# anti-aliasing and depth of field: its module is importlib.import_module("squigly-trace_amd.lens")
from .lens import Lens, LensFrame                                                    # noqa: F401
# motion blur: its module is importlib.import_module("squigly-trace_amd.shutter")
from .shutter import Motion                                                          # noqa: F401
# the display stage: its module is importlib.import_module("squigly-trace_amd.film")
from .film import Film, Glare                                                              # noqa: F401


def device_count() -> int:
    return lib().sq_device_count()


def release_cached_memory() -> None:
    """Hand the frame workspaces kept for the next scene back to the driver (sq_release_cached_memory)."""
    lib().sq_release_cached_memory()


def __getattr__(name):
    # torch is only needed for the resident-scene path
    if name in ("DeviceScene", "Progressive", "Adaptive", "AdaptiveLens", "Hits", "Radiance", "frame_seeds", "rule_reference", "frame_size_error", "MAX_CALL_PIXELS",
                "MAX_WAVEFRONT_PIXELS"):
        from . import device
        return getattr(device, name)
    if name == "Temporal":               # the sequence driver; its module is importlib.import_module("squigly-trace_amd.temporal")
        from . import temporal
        return temporal.Temporal
    if name in ("dist",):
        import importlib
        return importlib.import_module(__name__ + ".dist")
    raise AttributeError(name)
