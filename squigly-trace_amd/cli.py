"""Command line mirroring the reference's `squigly-trace` executable (app/Main.hs:13-75).

    python -m squigly-trace_amd.cli --samples 100 --dimensions 540,540 --savepath render/result.png

Flags and defaults are the reference's (cmdargs long names; `-s -d -p -c` short names as declared in
app/Main.hs:15-23).  The material file named by `mtllib` is read from ./data/, as in src/Obj.hs:52.
"""
import argparse
import os
import sys
import time

from . import BIH, Lens, Mesh, Motion, Settings, camera_from_text, lib, load_camera, render, render_adaptive, render_lens_rgb8, render_moving_sequence, render_progressive, render_sequence, render_views_rgb8, write_png
from ._native import SquiglyError


def parse_dimensions(text):
    try:
        w, h = (int(v) for v in text.strip("()").split(","))
    except ValueError:
        raise argparse.ArgumentTypeError("expected W,H")
    return (w, h)


def positive_int(text):
    try:
        v = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError("expected a positive integer")
    if v < 1:
        raise argparse.ArgumentTypeError("expected a positive integer")
    return v


def nonneg_float(text):
    try:
        v = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError("expected a number >= 0")
    if not v >= 0:
        raise argparse.ArgumentTypeError("expected a number >= 0")
    return v


def positive_float(text):
    try:
        v = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError("expected a number > 0")
    if not v > 0:
        raise argparse.ArgumentTypeError("expected a number > 0")
    return v


def unit_float(text):
    try:
        v = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError("expected a number in 0..1")
    if not 0 <= v <= 1:
        raise argparse.ArgumentTypeError("expected a number in 0..1")
    return v


def finite_nonneg_float(text):
    v = nonneg_float(text)
    if v == float("inf"):
        raise argparse.ArgumentTypeError("expected a finite number >= 0")
    return v


def finite_positive_float(text):
    v = positive_float(text)
    if v == float("inf"):
        raise argparse.ArgumentTypeError("expected a finite number > 0")
    return v


def path_depth(text):
    try:
        v = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError("expected an integer in 1..8")
    if not 1 <= v <= 8:
        raise argparse.ArgumentTypeError("expected an integer in 1..8")
    return v


def lattice_stride(text):
    try:
        v = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError("expected an integer in 1..16")
    if not 1 <= v <= 16:
        raise argparse.ArgumentTypeError("expected an integer in 1..16")
    return v


def parse_light(text):
    """A point light of --light: X,Y,Z (power 2, the reference's), X,Y,Z,P or X,Y,Z,R,G,B -> ((x, y, z), (r, g, b)).  The value may
    stand in parentheses, (X,Y,Z), which keeps a negative X from looking like an option on the command line."""
    try:
        v = [float(t) for t in text.strip("()").split(",")]
    except ValueError:
        v = []
    if len(v) not in (3, 4, 6):
        raise argparse.ArgumentTypeError("expected X,Y,Z or X,Y,Z,P or X,Y,Z,R,G,B")
    power = (2.0, 2.0, 2.0) if len(v) == 3 else (v[3],) * 3 if len(v) == 4 else tuple(v[3:])
    return (tuple(v[:3]), power)


def parse_sky(text):
    """The sky of --sky: R,G,B (a constant sky) or R,G,B,R,G,B (up, then down) -> ((r, g, b), (r, g, b)).  The value may stand in
    parentheses, as with --light."""
    try:
        v = [float(t) for t in text.strip("()").split(",")]
    except ValueError:
        v = []
    if len(v) not in (3, 6):
        raise argparse.ArgumentTypeError("expected R,G,B or R,G,B,R,G,B")
    return (tuple(v[:3]), tuple(v[3:]) if len(v) == 6 else tuple(v[:3]))


def parse_views(text):
    """The cameras of a views file: the reference's camera format (src/Obj.hs:60-70) repeated, each pair of non-blank lines one
    camera (position, then rotation angles).  Raises ValueError for an odd line count, a line that does not parse or no camera."""
    lines = [ln.strip() for ln in text.splitlines() if ln.strip()]
    if not lines:
        raise ValueError("no camera in the views file")
    if len(lines) % 2:
        raise ValueError(f"{len(lines)} non-blank lines: a camera is two lines (position, rotation)")
    cams = []
    for i in range(0, len(lines), 2):
        for ln in lines[i:i + 2]:
            try:
                ok = len([float(v) for v in ln.split()]) == 3
            except ValueError:
                ok = False
            if not ok:
                raise ValueError(f"camera {i // 2}: expected three numbers, got {ln!r}")
        try:
            cams.append(camera_from_text((lines[i] + "\n" + lines[i + 1] + "\n").encode()))
        except SquiglyError as e:
            raise ValueError(f"camera {i // 2}: {e}")
    return cams


def views_file(path):
    try:
        with open(path) as f:
            text = f.read()
    except OSError as e:
        raise argparse.ArgumentTypeError(f"cannot read {path}: {e}")
    try:
        return parse_views(text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(f"{path}: {e}")


def poses_file(path):
    """--poses: a float array [frames, materials, 3, 4] from a .npy file (never a pickle)."""
    import numpy as np
    try:
        poses = np.load(path, allow_pickle=False)
    except (OSError, ValueError) as e:
        raise argparse.ArgumentTypeError(f"cannot read {path}: {e}")
    if poses.ndim != 4 or poses.shape[2:] != (3, 4) or poses.dtype.kind != "f" or not np.isfinite(poses).all():
        raise argparse.ArgumentTypeError(f"{path}: expected a finite float array of shape [frames, materials, 3, 4], got "
                                         f"{poses.dtype} {poses.shape}")
    return poses


def history_clamp(text):
    """--history-clamp K[,RADIUS] as Temporal's clamp: (k, radius)."""
    parts = text.split(",")
    try:
        k, radius = float(parts[0]), (int(parts[1]) if len(parts) == 2 else 1)
        if len(parts) > 2 or not k >= 0 or not 1 <= radius <= 3:
            raise ValueError
    except ValueError:
        raise argparse.ArgumentTypeError("expected K[,RADIUS] with K >= 0 and RADIUS in 1..3")
    return k, radius


def view_paths(save_path, n):
    """Where the CLI writes the images of n views: <savepath stem>_<i:04d><ext>."""
    stem, ext = os.path.splitext(save_path)
    return [f"{stem}_{i:04d}{ext}" for i in range(n)]


def build_parser():
    p = argparse.ArgumentParser(prog="squigly-trace", description="A cute raytracer",
                                epilog="squigly-trace was made by Ruko (https://github.com/rukokarasu/)")
    p.add_argument("-s", "--samples", type=int, default=10, help="How many samples per pixel to trace")
    p.add_argument("-d", "--dimensions", type=parse_dimensions, default=(540, 540),
                   help="Dimensions of the resulting image")
    p.add_argument("-p", "--savepath", default="./render/result.png", help="Where to save the output")
    p.add_argument("--objpath", default="./data/scene.obj", help="File to load .obj from")
    p.add_argument("-c", "--camerapath", default="./data/camera", help="File to load camera data from")
    p.add_argument("--debug", action="store_true", help="Run in debug mode")
    p.add_argument("--debugpath", default="", help="File to write debug info to")
    p.add_argument("--cast", action="store_true", help="Raycast instead of raytracing (i.e. don't bounce rays)")
    # not a flag of the reference: progressive previews (the final image is the same bytes as without it)
    p.add_argument("--preview-every", type=positive_int, default=None, metavar="K",
                   help="Overwrite the savepath with a preview after every K samples (default: no previews)")
    p.add_argument("--views", type=views_file, default=None, metavar="FILE",
                   help="Render every camera of FILE (pairs of camera lines) in one call into <savepath stem>_<i:04d><ext>; "
                        "-c is not read")
    # not flags of the reference either: adaptive sampling (pixels stop once the stopping rule calls them done)
    p.add_argument("--adaptive", type=nonneg_float, default=None, metavar="TOL",
                   help="Adaptive sampling: a pixel stops once the standard error of its mean colour is at most TOL times "
                        "its colour (plus --adaptive-eps); a heuristic, --adaptive-first is its guard")
    p.add_argument("--adaptive-first", type=positive_int, default=8, metavar="N", help="Samples every pixel gets before the rule is asked (default 8)")
    p.add_argument("--adaptive-step", type=positive_int, default=8, metavar="N", help="Samples per later step (default 8)")
    p.add_argument("--adaptive-eps", type=nonneg_float, default=1.0, metavar="E", help="Absolute floor of the rule, in squared radiance per channel (default 1.0)")
    p.add_argument("--counts", default=None, metavar="FILE", help="With --adaptive: write the per-pixel sample counts to FILE (.npy, int32)")
    p.add_argument("--denoise", type=positive_float, nargs="?", const=True, default=None, metavar="SIGMA_L",
                   help="With --adaptive: filter the finished frame on the device, guided by its first hits and its own variance; "
                        "SIGMA_L is the luminance stop in standard deviations (default 4)")
    # not a flag of the reference: where the light of --cast is (the reference's is fixed at 0,3,-1 with power 2)
    p.add_argument("--light", type=parse_light, action="append", default=None, metavar="X,Y,Z[,P|,R,G,B]",
                   help="With --cast: a point light at X,Y,Z with power P (default 2) or R,G,B; repeat for several lights, "
                        "added in the order given (default: one light at 0,3,-1). A value that starts with a minus sign "
                        "is written --light=-1,2,3 or --light '(-1,2,3)'")
    # not a flag of the reference: how many rays long a path is (the reference's is fixed at 3)
    p.add_argument("--depth", type=path_depth, default=None, metavar="N",
                   help="Rays per path, 1..8: 1 = emission only, 2 = direct light, 3 = the reference's (default); not with --cast")
    # not a flag of the reference: what a ray that leaves the scene sees (the reference's is black)
    p.add_argument("--sky", type=parse_sky, default=None, metavar="R,G,B[,R,G,B]",
                   help="Radiance of a ray that leaves the scene: looking up (+z), then looking down (-z; default the same: "
                        "a constant sky), blended by the ray's direction (default: none, black); not with --cast")
    # not flags of the reference: a pixel integrates over its area, and the camera can have an aperture (include/squigly_lens.h)
    p.add_argument("--aa", type=unit_float, nargs="?", const=1.0, default=None, metavar="J",
                   help="Anti-aliasing: every primary ray starts from a point drawn from a square of side J pixels (default 1: a box "
                        "filter over the pixel)")
    p.add_argument("--subrays", type=positive_int, default=None, metavar="R",
                   help="With --aa or --aperture: primary rays per pixel, a divisor of --samples (default: one per sample)")
    p.add_argument("--aperture", type=finite_nonneg_float, default=None, metavar="A",
                   help="Depth of field: radius of the lens in world units (default 0: a pinhole)")
    p.add_argument("--focus", type=finite_positive_float, default=None, metavar="F",
                   help="With --aperture: forward distance of the plane in focus (default 1)")
    # not flags of the reference: the camera moves while the shutter is open (include/squigly_shutter.h)
    p.add_argument("--shutter-camera", type=camera_text, default=None, metavar="FILE",
                   help="Motion blur: a camera file with the pose as the shutter closes; --camera is the pose as it opens, and the "
                        "primary rays of a pixel (--subrays) are as many consecutive instants in between")
    p.add_argument("--shutter-jitter", type=unit_float, default=None, metavar="T",
                   help="With --shutter-camera: how much of its own part of the exposure a primary ray's instant is drawn from, "
                        "0..1 (default 1)")
    # not flags of the reference: the frames of a camera move, accumulated from frame to frame (include/squigly_temporal.h)
    p.add_argument("--sequence", type=views_file, default=None, metavar="FILE",
                   help="Render every camera of FILE (pairs of camera lines, as for --views) as one frame of a sequence, --samples "
                        "samples each, into <savepath stem>_<i:04d><ext>; -c is not read")
    p.add_argument("--temporal", type=unit_float, nargs="?", const=True, default=None, metavar="ALPHA_MIN",
                   help="With --sequence: accumulate every frame over the frames before it, reprojected through its first hits; "
                        "ALPHA_MIN is the least weight of the new frame (default 0.1)")
    # geometry that moves rigidly from frame to frame, and the clamp that goes with it (sq_temporal_accumulate_moving_device)
    p.add_argument("--poses", type=poses_file, default=None, metavar="FILE.npy",
                   help="With --sequence --temporal: a float array [frames, materials, 3, 4], the pose [R | t] of every material of "
                        "the scene in every frame (world = R local + t); every frame's scene is built from the moved mesh and its "
                        "history is reprojected through the move")
    p.add_argument("--history-clamp", type=history_clamp, default=None, metavar="K[,RADIUS]",
                   help="With --sequence --temporal: hold the history's colour to K standard deviations around the mean of the frame's "
                        "(2 RADIUS + 1)^2 neighbourhood before it is blended (RADIUS 1..3, default 1)")
    # not a flag of the reference: sparse frames (include/squigly_denoise.h: the lattice moves from frame to frame)
    p.add_argument("--sparse", type=lattice_stride, default=None, metavar="S",
                   help="With --sequence: trace only every S-th pixel of every S-th row of a frame (1..16; the lattice moves from "
                        "frame to frame) and the pixels no traced neighbour can stand for, and fill the rest in from their traced "
                        "neighbours on the same surface")
    # not flags of the reference: how the float frame becomes bytes, on the device (include/squigly_film.h).  They need a mode that
    # has such a frame on the device: --adaptive with --denoise, or --sequence
    p.add_argument("--film", choices=FILM_CURVES, default=None, metavar="CURVE",
                   help="With --adaptive --denoise or --sequence: the tone curve of the image, one of " + ", ".join(FILM_CURVES)
                        + " (default reference: the renderer's own bytes)")
    p.add_argument("--exposure", type=finite_positive_float, default=None, metavar="E", help="With --film: the frame is multiplied by E first (default 1)")
    p.add_argument("--auto-exposure", type=finite_positive_float, nargs="?", const=0.18, default=None, metavar="KEY",
                   help="With --film: meter every frame on the device and bring its median luminance to KEY (default 0.18); in a "
                        "--sequence the exposure follows from frame to frame")
    p.add_argument("--white", type=positive_float, default=None, metavar="W", help="With --film reinhard: the luminance that becomes white (default: none)")
    p.add_argument("--srgb", action="store_true", help="With --film other than reference: encode the image with the sRGB transfer function")
    p.add_argument("--dither", action="store_true", help="With --film other than reference: ordered 8 x 8 dither before the bytes are taken")
    # glare and white balance ahead of the curve (include/squigly_denoise.h: sq_denoise_glare_device)
    p.add_argument("--bloom", type=finite_nonneg_float, nargs="?", const=0.1, default=None, metavar="STRENGTH",
                   help="With --film other than reference: add the glare of what is brighter than --bloom-threshold to the frame, "
                        "at STRENGTH (default 0.1)")
    p.add_argument("--bloom-threshold", type=finite_nonneg_float, default=None, metavar="T",
                   help="With --bloom: the exposed luminance above which a pixel glares (default 1)")
    p.add_argument("--bloom-levels", type=bloom_levels, default=None, metavar="N", help="With --bloom: levels of the glare's pyramid, 1..8 (default 5)")
    p.add_argument("--white-balance", type=parse_balance, default=None, metavar="R,G,B",
                   help="With --film other than reference: multiply the frame's channels by R, G and B before the curve. A value that "
                        "starts with a minus sign is written --white-balance=-1,2,3 or --white-balance '(-1,2,3)'")
    return p


def bloom_levels(text):
    try:
        v = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError("expected an integer in 1..8")
    if not 1 <= v <= 8:
        raise argparse.ArgumentTypeError("expected an integer in 1..8")
    return v


def parse_balance(text):
    """The factors of --white-balance: R,G,B, in parentheses or not -> (r, g, b)."""
    try:
        v = [float(t) for t in text.strip("()").split(",")]
    except ValueError:
        v = []
    if len(v) != 3:
        raise argparse.ArgumentTypeError("expected R,G,B")
    return tuple(v)


BLOOM_CEILING = 16.0                         # what a glaring value saturates at, in thresholds (a threshold of 0: in units of 1)


def glare_of(a):
    """The Glare of --bloom and the flags that go with it, or None without --bloom."""
    if a.bloom is None:
        return None
    from .film import Glare
    t = 1.0 if a.bloom_threshold is None else a.bloom_threshold
    return Glare(threshold=t, ceiling=BLOOM_CEILING * (t if t > 0 else 1.0), levels=5 if a.bloom_levels is None else a.bloom_levels,
                 strength=a.bloom)


FILM_CURVES = ("reference", "atan", "reinhard", "filmic", "linear")
AUTO_EXPOSURE_RATE = 0.25                    # of a --sequence: how far the exposure moves towards a frame's target


def film_of(a):
    """The Film of --film and the flags that go with it, or None without them."""
    if a.film is None:
        return None
    from .film import Film, srgb_lut
    auto = None
    if a.auto_exposure is not None:
        auto = dict(key=a.auto_exposure, rate=AUTO_EXPOSURE_RATE if a.sequence is not None else 1.0)
    return Film(curve=a.film, exposure=1.0 if a.exposure is None else a.exposure, white=float("inf") if a.white is None else a.white,
                lut=srgb_lut() if a.srgb else None, dither=a.dither, auto=auto, glare=glare_of(a), balance=a.white_balance)


def camera_text(path):
    """The text of a camera file, checked to be one."""
    try:
        with open(path, "rb") as f:
            text = f.read()
        camera_from_text(text)
    except Exception as e:                                      # a missing file, or whatever the library says about its text
        raise argparse.ArgumentTypeError(f"{path}: {e}")
    return text


def lens_of(a):
    """The Lens of --aa / --aperture / --focus, or None when the frame has none of them; --shutter-camera alone means Lens(jitter=0)."""
    if a.aa is None and a.aperture is None:
        return Lens(jitter=0.0) if a.shutter_camera is not None else None
    return Lens(jitter=0.0 if a.aa is None else a.aa, aperture=a.aperture or 0.0, focus=1.0 if a.focus is None else a.focus)


def parse_args(argv=None):
    p = build_parser()
    a = p.parse_args(argv)
    if a.views is not None and a.preview_every is not None:
        p.error("--views cannot be combined with --preview-every")
    if a.adaptive is not None and (a.views is not None or a.preview_every is not None):
        p.error("--adaptive cannot be combined with --views or --preview-every")
    if a.counts is not None and a.adaptive is None:
        p.error("--counts needs --adaptive")
    if a.temporal is not None and a.sequence is None:
        p.error("--temporal needs --sequence")
    if a.temporal is not None and (a.adaptive is not None or a.aa is not None):
        p.error("--temporal cannot be combined with --adaptive or --aa")
    if a.sparse is not None and a.sequence is None:
        p.error("--sparse needs --sequence (a sparse frame's lattice moves from frame to frame)")
    for flag, given in (("--poses", a.poses is not None), ("--history-clamp", a.history_clamp is not None)):
        if given and (a.sequence is None or a.temporal is None):
            p.error(f"{flag} needs --sequence --temporal")
    if a.poses is not None:
        if a.sparse is not None:
            p.error("--poses cannot be combined with --sparse")
        if len(a.poses) != len(a.sequence):
            p.error(f"--poses holds {len(a.poses)} frames, --sequence {len(a.sequence)} cameras")
    if a.sequence is not None:
        for flag, given in (("--cast", a.cast), ("--views", a.views is not None), ("--adaptive", a.adaptive is not None),
                            ("--preview-every", a.preview_every is not None), ("--light", a.light is not None)):
            if given:
                p.error(f"--sequence cannot be combined with {flag}")
        if a.samples < 1:
            p.error("--sequence needs --samples >= 1")
    if a.denoise is not None and a.adaptive is None and a.sequence is None:
        p.error("--denoise needs --adaptive (the filter takes its variance from the adaptive frame's second moments)")
    film_flags = [flag for flag, given in (("--exposure", a.exposure is not None), ("--auto-exposure", a.auto_exposure is not None),
                                           ("--white", a.white is not None), ("--srgb", a.srgb), ("--dither", a.dither),
                                           ("--bloom", a.bloom is not None), ("--bloom-threshold", a.bloom_threshold is not None),
                                           ("--bloom-levels", a.bloom_levels is not None), ("--white-balance", a.white_balance is not None)) if given]
    if film_flags and a.film is None:
        p.error(f"{film_flags[0]} needs --film")
    if a.bloom is None and (a.bloom_threshold is not None or a.bloom_levels is not None):
        p.error("--bloom-threshold and --bloom-levels need --bloom")
    if a.film is not None:
        if a.sequence is None and (a.adaptive is None or a.denoise is None):
            p.error("--film needs a float frame on the device: --adaptive with --denoise, or --sequence")
        if a.film == "reference" and (a.srgb or a.dither):
            p.error("--film reference takes neither --srgb nor --dither (it is the renderer's own conversion to bytes)")
        if a.film == "reference" and (a.bloom is not None or a.white_balance is not None):
            p.error("--film reference takes neither --bloom nor --white-balance (it is the renderer's own conversion to bytes)")
        try:
            glare_of(a)
        except SquiglyError as e:
            p.error(f"--bloom: {e}")
        if a.white is not None and a.film != "reinhard":
            p.error("--white needs --film reinhard")
        if a.exposure is not None and a.auto_exposure is not None:
            p.error("--exposure cannot be combined with --auto-exposure")
    if a.light is not None and not a.cast:
        p.error("--light needs --cast")
    if a.depth is not None and a.cast:
        p.error("--depth cannot be combined with --cast (a cast image has no paths)")
    if a.sky is not None and a.cast:
        p.error("--sky cannot be combined with --cast (a cast image has no sky)")
    if a.shutter_jitter is not None and a.shutter_camera is None:
        p.error("--shutter-jitter needs --shutter-camera")
    if a.aa is None and a.aperture is None and a.shutter_camera is None:
        if a.subrays is not None:
            p.error("--subrays needs --aa, --aperture or --shutter-camera")
        if a.focus is not None:
            p.error("--focus needs --aperture")
    else:
        if a.focus is not None and a.aperture is None:
            p.error("--focus needs --aperture")
        for flag, given in (("--cast", a.cast), ("--views", a.views is not None), ("--adaptive", a.adaptive is not None),
                            ("--preview-every", a.preview_every is not None), ("--sequence", a.sequence is not None)):
            if given:
                p.error(f"--aa, --subrays, --aperture, --focus and --shutter-camera cannot be combined with {flag}")
        if a.samples < 1 or a.samples % (a.subrays or a.samples):
            p.error(f"--subrays must divide --samples (got {a.subrays} and {a.samples})")
    return a


def main(argv=None):
    a = parse_args(argv)
    settings = Settings(samples=a.samples, dimensions=a.dimensions, savePath=a.savepath, objPath=a.objpath,
                        cameraPath=a.camerapath, debug=a.debug, debugPath=a.debugpath, cast=a.cast)
    cam = load_camera(settings.cameraPath) if a.views is None and a.sequence is None else None   # app/Main.hs:38
    mesh = Mesh.from_obj(settings.objPath, "./data")            # loadTris, app/Main.hs:58-61 + src/Obj.hs:52
    if settings.debug:                                          # src/Obj.hs:55-57: print (head objs); print mats
        first, mats = mesh.debug_show()
        if not first:                                           # `head objs` of a file without objects throws in the reference
            print("squigly-trace: Prelude.head: empty list", file=sys.stderr)
            return 1
        print(first)
        print(mats)
    # loadBIH, app/Main.hs:63-75.  Both builds give the same arrays; the GPU one wins from a few 10^4 triangles up.
    bih = BIH(mesh, device=0 if (len(mesh) >= 50000 and lib().sq_device_count() > 0) else None)
    if settings.debug:
        if settings.debugPath:
            nodes = bih.nodes
            with open(settings.debugPath, "w") as f:            # flattened dump (the Haskell `show bih` text is not reproduced)
                f.write(f"BIH bounds={bih.bounds.tolist()} nodes={len(nodes)} tris={len(bih.tris)}\n")
                for i, nd in enumerate(nodes):
                    f.write(f"{i} kind={int(nd['kind']) & 3} count={int(nd['kind']) >> 2} lmax={nd['lmax']!r} "
                            f"rmin={nd['rmin']!r} link={int(nd['link'])}\n")
            print(f"Wrote BIH to {settings.debugPath}")
        print(f"BIH height is {bih.height}")
        print(f"Length of longest leaf is {bih.longest_leaf}")
        print(f"Number of leaves is {bih.num_leaves}")
    print("Rendering scene...")
    t0 = time.time()
    print("Started at " + time.strftime("%H:%M:%S%p UTC", time.gmtime(t0)).lower().replace("utc", "UTC"))
    os.makedirs(os.path.dirname(os.path.abspath(settings.savePath)), exist_ok=True)
    if a.views is not None:
        imgs = render_views_rgb8(bih, a.views, settings.samples, settings.dimensions, settings.cast, lights=a.light, depth=a.depth, sky=a.sky)
        for path, img in zip(view_paths(settings.savePath, len(imgs)), imgs):
            write_png(path, img)
        print(f"Wrote {len(imgs)} views to {view_paths(settings.savePath, 1)[0]} ...")
    elif a.sequence is not None:
        paths = view_paths(settings.savePath, len(a.sequence))
        more = {} if a.temporal is None or a.temporal is True else {"alpha_min": a.temporal}
        if a.poses is not None:
            frames = render_moving_sequence(mesh, a.sequence, a.poses, settings.samples, settings.dimensions, clamp=a.history_clamp,
                                            denoise=a.denoise, depth=a.depth, sky=a.sky, film=film_of(a), **more)
        else:
            frames = render_sequence(bih, a.sequence, settings.samples, settings.dimensions, temporal=a.temporal is not None, denoise=a.denoise,
                                     depth=a.depth, sky=a.sky, film=film_of(a), sparse=a.sparse, clamp=a.history_clamp, **more)
        for path, img in zip(paths, frames):
            write_png(path, img)
        print(f"Wrote {len(paths)} frames to {paths[0]} ...")
    elif a.adaptive is not None:
        import numpy as np
        for done, live, spent, img, counts in render_adaptive(bih, cam, settings.samples, settings.dimensions, a.adaptive, eps=a.adaptive_eps,
                                                              first=a.adaptive_first, step=a.adaptive_step, cast=settings.cast, lights=a.light,
                                                              depth=a.depth, sky=a.sky, denoise=a.denoise, film=film_of(a)):
            print(f"Adaptive {done}/{settings.samples} live {live} spent {spent}")
        if a.denoise is not None:
            print("Denoised")
        write_png(settings.savePath, img)
        if a.counts is not None:
            with open(a.counts, "wb") as f:                     # the name as given (np.save would append .npy to a path)
                np.save(f, counts.astype(np.int32))
    elif lens_of(a) is not None:
        motion = None
        if a.shutter_camera is not None:
            with open(settings.cameraPath, "rb") as f:
                motion = Motion(f.read(), a.shutter_camera, 1.0 if a.shutter_jitter is None else a.shutter_jitter)
        write_png(settings.savePath, render_lens_rgb8(bih, cam, settings.samples, settings.dimensions, lens=lens_of(a), subrays=a.subrays,
                                                      depth=a.depth, sky=a.sky, motion=motion))
    elif a.preview_every is None and a.light is None and a.depth is None and a.sky is None:
        render(bih, cam, settings)
    elif a.preview_every is None:                               # caller-given lights, depths and skies live on a resident scene: one step of all samples
        for _, img in render_progressive(bih, cam, settings.samples, settings.dimensions, settings.samples, settings.cast, lights=a.light,
                                         depth=a.depth, sky=a.sky):
            write_png(settings.savePath, img)
    else:
        for done, img in render_progressive(bih, cam, settings.samples, settings.dimensions, a.preview_every, settings.cast, lights=a.light,
                                            depth=a.depth, sky=a.sky):
            write_png(settings.savePath, img)
            print(f"Preview: {done}/{settings.samples} samples written to {settings.savePath}")
    t1 = time.time()
    print("Finished at " + time.strftime("%H:%M:%S%p UTC", time.gmtime(t1)).lower().replace("utc", "UTC"))
    print(f"Took {t1 - t0:.6f}s")
    return 0


if __name__ == "__main__":
    sys.exit(main())
