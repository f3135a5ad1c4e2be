"""Build the package's seven shared libraries (the table LIBS below: the renderer libsquigly_hip.so and, beside it, one library per
later stage) and the CLI in-tree with hipcc.

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

CLIENT_LINK = ["-L" + HERE, "-lsquigly_hip", "-Wl,-rpath,$ORIGIN"]
COMMON_HEADERS = ["sq_math.h", "sq_error.h", "sq_call_checks.h"]
LENS_HEADERS = COMMON_HEADERS + ["sq_lens_plan.h", "sq_lens_ray.h", "sq_lens_frame.h", "../../include/squigly_lens.h", "../../include/squigly_hip.h"]

LIBS = {}


def _library(name, sources, headers, client=False):
    """Adds a row to LIBS.  out: libsquigly_<name>.so beside this file; sources, headers: what its id is hashed over, under csrc/; macro:
    the -D that carries the id into the library (what sq_<name>_build_id() returns); salt: what the id's hash starts from, so that
    no two libraries share an id; link: behind the output -- a client is linked against libsquigly_hip.so's public C-ABI and built
    after it.  The main library is the one without a name of its own: libsquigly_hip.so, SQ_BUILD_ID, an empty salt."""
    tag = "" if name == "main" else name
    LIBS[name] = dict(out=os.path.join(HERE, "libsquigly_%s.so" % (tag or "hip")), sources=sources, headers=headers,
                      macro="SQ_%sBUILD_ID" % (tag.upper() + "_" if tag else ""), salt=(tag + "\0").encode() if tag else b"",
                      link=CLIENT_LINK if client else [])


# The seven libraries, in the order build() makes them.  Every one has the same FLAGS (its bits rest on -ffp-contract=off and the
# correctly rounded divide / sqrt as the renderer's do) and an id of its own: the main library's id -- and the counter files stamped
# with it -- do not move when another library changes.

# the denoiser (include/squigly_denoise.h): device images to device images; the arithmetic of a sparse frame's pixel
# (sq_upsample_pixel.h) and of the glare stage's (sq_glare_pixel.h) are its own
_library("denoise", ["sq_denoise.hip"], COMMON_HEADERS + ["sq_glare_pixel.h", "sq_upsample_pixel.h", "../../include/squigly_denoise.h"])
# the renderer: HIP kernels and the host side (include/squigly_hip.h, include/squigly_host.h); build() makes the CLI with it
_library("main", ["sq_device.hip", "sq_bih_device.hip", "sq_host.cpp"],
         COMMON_HEADERS + ["sq_scene.h", "sq_layout.h", "sq_pack.h", "sq_plan.h", "sq_host_types.h", "sq_cull_lemma.h", "sq_pack_level1.h",
                           "sq_pack_scene.h", "sq_plan_call.h", "sq_frame.h", "sq_kernels_lane.h", "sq_kernels_wave.h", "sq_kernels_trace.h",
                           "cli_main.cpp", "../../include/squigly_hip.h", "../../include/squigly_host.h"])
# jittered, thin-lens primary rays (include/squigly_lens.h)
_library("lens", ["sq_lens.hip"], LENS_HEADERS, client=True)
# the lens frame for the live pixels of a mask (include/squigly_mlens.h): shares the planner, a sub-ray's arithmetic and the
# frame's kernels and batch loop with the lens library as headers, not as symbols
_library("mlens", ["sq_mlens.hip"], LENS_HEADERS + ["../../include/squigly_mlens.h"], client=True)
# motion blur (include/squigly_shutter.h): the lens libraries' headers as text; the pose of an instant (sq_shutter_pose.h) is its own
_library("shutter", ["sq_shutter.hip"], LENS_HEADERS + ["sq_shutter_pose.h", "../../include/squigly_shutter.h"], client=True)
# temporal accumulation (include/squigly_temporal.h): device images to device images like the denoiser; no client of the main
# library, whose header it reads for sq_camera alone; the arithmetic of a pixel (sq_temporal_pixel.h) is its own
_library("temporal", ["sq_temporal.hip"], COMMON_HEADERS + ["sq_temporal_pixel.h", "../../include/squigly_temporal.h", "../../include/squigly_hip.h"])
# the display stage (include/squigly_film.h): device images to device images, no client; the arithmetic of a pixel
# (sq_film_pixel.h) is its own, and sq_math.h is read for the reference's tonemap
_library("film", ["sq_film.hip"], COMMON_HEADERS + ["sq_film_pixel.h", "../../include/squigly_film.h"])


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
    """Compiles a row of LIBS.  out: an experimental variant (extra options) beside the product library; SQ_LIB_PATH / SQ_LENS_LIB_PATH /
    SQ_MLENS_LIB_PATH / SQ_SHUTTER_LIB_PATH select one at load time, and film.load(path) loads one beside the product's."""
    out = out or lib["out"]
    subprocess.check_call([hipcc()] + FLAGS + list(extra) + ['-D%s="%s"' % (lib["macro"], lib_source_id(lib, extra)), "-x", "hip"]
                          + [os.path.join(CSRC, s) for s in lib["sources"]] + ["-o", out] + lib["link"])
    return out


def hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    raise RuntimeError("hipcc not found")


def source_id(extra=()):
    """The main library's id (tools/collect_profiles.py, bench.py's result line)."""
    return lib_source_id(LIBS["main"], extra)


def stale():
    return lib_stale(LIBS["main"])


def compile_cli():
    """The reference's executable (app/Main.hs) over the C-ABI.  Its --depth path copies a device frame back: the HIP runtime's host
    API, from the ROCm tree hipcc belongs to."""
    import shutil
    os.makedirs(os.path.dirname(CLI), exist_ok=True)
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(shutil.which(hipcc()) or hipcc())))
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                           os.path.join(CSRC, "cli_main.cpp"), "-o", CLI,
                           "-L" + HERE, "-lsquigly_hip", "-L" + os.path.join(rocm, "lib"), "-lamdhip64", "-Wl,-rpath,$ORIGIN/..", "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath," + os.path.join(rocm, "lib"),
                           "-Wl,--allow-shlib-undefined"])


def build(force=False, extra=(), out=None):
    """Every library of LIBS that does not carry its current id (force: every one), in the table's order, and the CLI with the main
    library; extra goes to the main library alone.  out: a variant of the main library beside the product, and nothing else."""
    if out is not None:
        return compile_lib(LIBS["main"], extra, out)
    for name, lib in LIBS.items():
        main = name == "main"
        if force or lib_stale(lib) or (main and not os.path.exists(CLI)):
            compile_lib(lib, extra if main else ())
            if main:
                compile_cli()
    return OUT


if __name__ == "__main__":
    outs = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--out=")]
    # -Dname[=v] / -Rpass / -save-temps go to hipcc as they are; --flag=<anything> passes <anything> (e.g. --flag=-mllvm --flag=-amdgpu-skip-threshold=24)
    print(build(force="--force" in sys.argv, extra=[a for a in sys.argv[1:] if a[:2] in ("-R", "-D") or a.startswith("-save")] + [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--flag=")],
                out=os.path.join(HERE, outs[0]) if outs else None))
