"""Build libsquigly_hip.so (HIP kernels for gfx950 + host side), libsquigly_denoise.so (the denoiser), libsquigly_lens.so (jittered,
thin-lens primary rays), libsquigly_mlens.so (those rays for the live pixels of a mask), libsquigly_shutter.so (those rays, dense
or listed, under a camera that moves during the exposure), libsquigly_temporal.so (temporal accumulation over a sequence of
frames) and libsquigly_film.so (exposure, tone curve and quantisation of a frame) in-tree with hipcc.

    python squigly-trace_amd/build.py [--force]

The flags that matter for bit-exact parity with the CPU oracle:
  -ffp-contract=off                               no FMA contraction (host and device)
  -fhip-fp32-correctly-rounded-divide-sqrt        IEEE fp32 divide / sqrt on the device
  -fno-slp-vectorize                              performance only: packed fp32 VALU ops are slow on gfx950
  no -ffast-math, denormals kept (hipcc default for gfx9)
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT = os.path.join(HERE, "libsquigly_hip.so")
SOURCES = ["sq_device.hip", "sq_bih_device.hip", "sq_host.cpp"]
HEADERS = ["sq_math.h", "sq_error.h", "sq_call_checks.h", "sq_scene.h", "sq_layout.h", "sq_pack.h", "sq_plan.h", "sq_host_types.h", "sq_cull_lemma.h", "sq_pack_level1.h", "sq_pack_scene.h", "sq_plan_call.h", "sq_frame.h", "sq_kernels_lane.h", "sq_kernels_wave.h", "sq_kernels_trace.h", "cli_main.cpp", "../../include/squigly_hip.h", "../../include/squigly_host.h"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
         "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-fast-math",
         # v_pk_mul_f32 / v_pk_add_f32 issue at ~9.5 cycles per wave on gfx950 against ~2.6 for the scalar forms
         # (tools/ubench/valu_rate.hip): keep the SLP vectoriser from packing the fp32 vector math.
         "-fno-slp-vectorize",
         # performance only (scheduling; bits unchanged): the trace kernel is bound by the latency of its dependent steps
         # at 4 waves per SIMD, and the ILP-first machine scheduler measured -0.5 ... -1.3 % on all three scenes against
         # the default (same gpurun call, tools/ab_variant.sh); max-memory-clause +-0, iterative-minreg +2 %
         "-mllvm", "-amdgpu-sched-strategy=max-ilp",
         "-Wall", "-Wno-unused-function"]


CLI = os.path.join(HERE, "bin", "squigly-trace")

# The second library: the denoiser (include/squigly_denoise.h).  One source, the same FLAGS (its bits rest on -ffp-contract=off and
# the correctly rounded divide / sqrt as the renderer's do) and an id of its own: the main library's id -- and the counter files
# stamped with it -- do not move when the filter changes.
DENOISE_OUT = os.path.join(HERE, "libsquigly_denoise.so")
DENOISE_SOURCES = ["sq_denoise.hip"]
DENOISE_HEADERS = ["sq_math.h", "sq_error.h", "sq_call_checks.h", "../../include/squigly_denoise.h"]

# The third library: jittered, thin-lens primary rays (include/squigly_lens.h).  A client of libsquigly_hip.so's public C-ABI: it is
# linked against that library and built after it, with the same FLAGS and an id of its own.
LENS_OUT = os.path.join(HERE, "libsquigly_lens.so")
LENS_SOURCES = ["sq_lens.hip"]
LENS_HEADERS = ["sq_math.h", "sq_error.h", "sq_call_checks.h", "sq_lens_plan.h", "sq_lens_ray.h", "sq_lens_frame.h", "../../include/squigly_lens.h",
                "../../include/squigly_hip.h"]

# The fourth library: the lens frame for the live pixels of a mask (include/squigly_mlens.h).  A client of libsquigly_hip.so like the
# lens library, with which it shares the planner, a sub-ray's arithmetic and the frame's kernels and batch loop (sq_lens_plan.h,
# sq_lens_ray.h, sq_lens_frame.h) as headers, not as symbols.
MLENS_OUT = os.path.join(HERE, "libsquigly_mlens.so")
MLENS_SOURCES = ["sq_mlens.hip"]
MLENS_HEADERS = LENS_HEADERS + ["../../include/squigly_mlens.h"]

# The fifth library: motion blur (include/squigly_shutter.h).  A client of libsquigly_hip.so like the two lens libraries, whose headers
# it shares as text, not as symbols; the pose of an instant (sq_shutter_pose.h) is its own.
SHUTTER_OUT = os.path.join(HERE, "libsquigly_shutter.so")
SHUTTER_SOURCES = ["sq_shutter.hip"]
SHUTTER_HEADERS = LENS_HEADERS + ["sq_shutter_pose.h", "../../include/squigly_shutter.h"]

# The sixth library: temporal accumulation (include/squigly_temporal.h).  Like the denoiser it maps device images to device images
# and is not linked against the main library, whose header it reads for sq_camera alone; the arithmetic of a pixel
# (sq_temporal_pixel.h) is its own.
TEMPORAL_OUT = os.path.join(HERE, "libsquigly_temporal.so")
TEMPORAL_SOURCES = ["sq_temporal.hip"]
TEMPORAL_HEADERS = ["sq_math.h", "sq_error.h", "sq_call_checks.h", "sq_temporal_pixel.h", "../../include/squigly_temporal.h",
                    "../../include/squigly_hip.h"]

# The seventh library: the display stage (include/squigly_film.h).  Device images to device images like the denoiser and the temporal
# library, and no client of the main library; the arithmetic of a pixel (sq_film_pixel.h) is its own, and sq_math.h is read for the
# reference's tonemap.
FILM_OUT = os.path.join(HERE, "libsquigly_film.so")
FILM_SOURCES = ["sq_film.hip"]
FILM_HEADERS = ["sq_math.h", "sq_error.h", "sq_call_checks.h", "sq_film_pixel.h", "../../include/squigly_film.h"]

# One description per library.  macro: the -D that carries the id into the library (what sq_build_id(), sq_denoise_build_id(),
# sq_lens_build_id(), sq_mlens_build_id(), sq_shutter_build_id(), sq_temporal_build_id() and sq_film_build_id() return); salt: what the id's hash starts from, so that no two libraries share an id; link: behind the output.
MAIN = dict(out=OUT, sources=SOURCES, headers=HEADERS, macro="SQ_BUILD_ID", salt=b"", link=[])
DENOISE = dict(out=DENOISE_OUT, sources=DENOISE_SOURCES, headers=DENOISE_HEADERS, macro="SQ_DENOISE_BUILD_ID", salt=b"denoise\0", link=[])
LENS = dict(out=LENS_OUT, sources=LENS_SOURCES, headers=LENS_HEADERS, macro="SQ_LENS_BUILD_ID", salt=b"lens\0",
            link=["-L" + HERE, "-lsquigly_hip", "-Wl,-rpath,$ORIGIN"])
MLENS = dict(out=MLENS_OUT, sources=MLENS_SOURCES, headers=MLENS_HEADERS, macro="SQ_MLENS_BUILD_ID", salt=b"mlens\0", link=LENS["link"])
SHUTTER = dict(out=SHUTTER_OUT, sources=SHUTTER_SOURCES, headers=SHUTTER_HEADERS, macro="SQ_SHUTTER_BUILD_ID", salt=b"shutter\0", link=LENS["link"])
TEMPORAL = dict(out=TEMPORAL_OUT, sources=TEMPORAL_SOURCES, headers=TEMPORAL_HEADERS, macro="SQ_TEMPORAL_BUILD_ID", salt=b"temporal\0", link=[])
FILM = dict(out=FILM_OUT, sources=FILM_SOURCES, headers=FILM_HEADERS, macro="SQ_FILM_BUILD_ID", salt=b"film\0", link=[])


def lib_source_id(lib, extra=()):
    """First 16 hex digits of SHA-256 over the library's salt, every source and header of it, the flags and the extra options: the
    main library's is also what tools/collect_profiles.py stamps its counter files with."""
    import hashlib
    h = hashlib.sha256(lib["salt"])
    for f in sorted(lib["sources"] + lib["headers"]):
        h.update(f.encode() + b"\0")
        with open(os.path.join(CSRC, f), "rb") as fh:
            h.update(fh.read())
    h.update("\0".join(FLAGS + sorted(extra)).encode())
    return h.hexdigest()[:16]


def lib_stale(lib):
    """True unless the in-tree library was built from exactly the sources, headers and flags that are here now: it must carry the
    current id (file times can lie after a checkout or a copy, and say nothing the id does not)."""
    if not os.path.exists(lib["out"]):
        return True
    with open(lib["out"], "rb") as f:
        return lib_source_id(lib).encode() not in f.read()


def compile_lib(lib, extra=(), out=None):
    """out: an experimental variant (extra options) beside the product library; SQ_LIB_PATH / SQ_LENS_LIB_PATH / SQ_MLENS_LIB_PATH / SQ_SHUTTER_LIB_PATH select it at load time."""
    out = out or lib["out"]
    subprocess.check_call([hipcc()] + FLAGS + list(extra) + ['-D%s="%s"' % (lib["macro"], lib_source_id(lib, extra)), "-x", "hip"]
                          + [os.path.join(CSRC, s) for s in lib["sources"]] + ["-o", out] + lib["link"])
    return out


def hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    raise RuntimeError("hipcc not found")


def source_id(extra=()): return lib_source_id(MAIN, extra)
def stale(): return lib_stale(MAIN)
def denoise_source_id(): return lib_source_id(DENOISE)
def lens_source_id(extra=()): return lib_source_id(LENS, extra)
def lens_stale(): return lib_stale(LENS)
def mlens_source_id(extra=()): return lib_source_id(MLENS, extra)
def mlens_stale(): return lib_stale(MLENS)
def shutter_source_id(extra=()): return lib_source_id(SHUTTER, extra)
def shutter_stale(): return lib_stale(SHUTTER)
def temporal_source_id(): return lib_source_id(TEMPORAL)
def temporal_stale(): return lib_stale(TEMPORAL)
def film_source_id(extra=()): return lib_source_id(FILM, extra)
def film_stale(): return lib_stale(FILM)


def build_client(lib, force=False, extra=(), out=None):
    """A client library of libsquigly_hip.so: compiled unless it is the in-tree product and carries the current id."""
    if out is None and not force and not lib_stale(lib):
        return lib["out"]
    return compile_lib(lib, extra, out)


def build_lens(force=False, extra=(), out=None): return build_client(LENS, force, extra, out)
def build_mlens(force=False, extra=(), out=None): return build_client(MLENS, force, extra, out)
def build_shutter(force=False, extra=(), out=None): return build_client(SHUTTER, force, extra, out)


def build_temporal(force=False):
    """The temporal library: compiled unless the in-tree product carries the current id.  (No client of the main library.)"""
    return build_client(TEMPORAL, force)


def build_film(force=False, extra=(), out=None):
    """The film library: compiled unless the in-tree product carries the current id.  (No client of the main library.)  extra, out:
    a variant beside it, e.g. -DSQ_FILM_HIST_FOLD=0 (tools/gpu_film.py measures the histogram's folding forms that way)."""
    return build_client(FILM, force, extra, out)


def build(force=False, extra=(), out=None):
    if out is not None:
        return compile_lib(MAIN, extra, out)
    if force or lib_stale(DENOISE):
        compile_lib(DENOISE)
    if force or lib_stale(MAIN) or not os.path.exists(CLI):
        compile_lib(MAIN, extra)
        # the reference's executable (app/Main.hs) over the C-ABI
        os.makedirs(os.path.dirname(CLI), exist_ok=True)
        # (its --depth path copies a device frame back: the HIP runtime's host API, from the ROCm tree hipcc belongs to)
        import shutil
        rocm = os.path.dirname(os.path.dirname(os.path.realpath(shutil.which(hipcc()) or hipcc())))
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                               os.path.join(CSRC, "cli_main.cpp"), "-o", CLI,
                               "-L" + HERE, "-lsquigly_hip", "-L" + os.path.join(rocm, "lib"), "-lamdhip64", "-Wl,-rpath,$ORIGIN/..", "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath," + os.path.join(rocm, "lib"),
                               "-Wl,--allow-shlib-undefined"])
    build_lens(force)
    build_mlens(force)
    build_shutter(force)
    build_temporal(force)
    build_film(force)
    return OUT


if __name__ == "__main__":
    outs = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--out=")]
    # -Dname[=v] / -Rpass / -save-temps go to hipcc as they are; --flag=<anything> passes <anything> (e.g. --flag=-mllvm --flag=-amdgpu-skip-threshold=24)
    print(build(force="--force" in sys.argv, extra=[a for a in sys.argv[1:] if a[:2] in ("-R", "-D") or a.startswith("-save")] + [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--flag=")],
                out=os.path.join(HERE, outs[0]) if outs else None))
