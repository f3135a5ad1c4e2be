"""Option tables and kernel forms of the GPU tests: what a test puts a DeviceScene back to, and the option sets it walks.

Belongs here: a table of option defaults, the one function that applies a table, its depth and sky layers, and the lists of
(options, expected form) that several test modules parametrise over.  A table lists the keys its tests change, each at the library's
own default (Options in csrc/sq_plan.h; tests/test_plan.py holds every table to it), so `set_options(ds, TABLE)` undoes whatever
`set_options(ds, TABLE, **opts)` did.  Three options stay out of every table: `timing` and `rng_table_mb` (tests that need them set
and restore them by hand), and `aux_low_priority`, whose setting synchronises and destroys the scene's second stream."""
import os

THREADS = min(os.cpu_count() or 1, 16)                  # of an oracle render
DEFAULT_SLOTS = 512 << 20

# frames in sample ranges, masked frames (progressive, adaptive, slot fates)
FRAME = {"variant": 2, "resident": 1, "profile": 0, "overlap": 0, "primary_pooled": 0, "pool": 1, "slots": DEFAULT_SLOTS}
# multi-view frames
VIEWS = {**FRAME, "cull": 1}
# intersection queries
RAY_QUERY = {"variant": 2, "resident": 1, "pool": 1, "trace_blocks_per_cu": 0, "profile": 0, "cull": 1, "slots": DEFAULT_SLOTS}
# radiance queries and the frames they are compared with; under the depth and sky layers too
RADIANCE = {**RAY_QUERY, "overlap": 0, "primary_pooled": 0, "primary_resident": 1, "pixel_major": -1}
# cast frames under lights, and every stream-taking call
CAST = {"variant": 2, "resident": 1, "pool": 1, "overlap": 0, "cast_wavefront": 0, "primary_pooled": 0, "slots": DEFAULT_SLOTS}
TABLES = {"FRAME": FRAME, "VIEWS": VIEWS, "RAY_QUERY": RAY_QUERY, "RADIANCE": RADIANCE, "CAST": CAST}


def set_options(ds, table, **opts):
    """Every key of the table at its default, but those of opts as given; in the table's order."""
    for k, v in {**table, **opts}.items():
        ds.set_option(k, v)


def set_depth_options(ds, depth=3, deep=0, **opts):
    """RADIANCE, the generic-depth switch, no cast wavefront, and the scene's path depth."""
    set_options(ds, RADIANCE, **opts)
    ds.set_option("deep", deep)
    ds.set_option("cast_wavefront", 0)
    ds.set_depth(depth)


def set_sky_options(ds, sky=None, depth=3, deep=0, **opts):
    """set_depth_options, and the scene's sky: None, or (up, down)."""
    set_depth_options(ds, depth=depth, deep=deep, **opts)
    if sky is None:
        ds.set_sky(None)
    else:
        ds.set_sky(*sky)


# ---- forms -------------------------------------------------------------------------------------------------------------------
# (options, expected trace form) of data/scene.obj
SCENE_FORMS = (({"variant": 1}, "per_pixel"), ({}, "resident"), ({"pool": 0}, "resident"),
               ({"resident": 0, "trace_blocks_per_cu": 3}, "streaming_six_wave"), ({"resident": 0, "trace_blocks_per_cu": 1}, "streaming_plain"),
               ({"resident": 0, "pool": 0}, "streaming_plain"), ({"profile": 1}, "resident"))
FORM_IDS = [f"{f}-{'-'.join(f'{k}{v}' for k, v in o.items()) or 'default'}" for o, f in SCENE_FORMS]
# (options, expected primary form) of a wavefront frame
PRIMARY_FORMS = (({}, "resident"), ({"primary_resident": 0}, "per_lane"), ({"primary_pooled": 1}, "pooled"), ({"variant": 1}, "none"))
# the option tuples test_kernel_variants_agree walks: (variant, resident, profile, overlap, primary_pooled)
OPTION_TUPLES = ((1, 1, 0, 0, 0), (2, 1, 0, 0, 0), (2, 0, 0, 0, 0), (2, 1, 1, 0, 0), (2, 0, 1, 0, 0), (2, 1, 0, 1, 0), (2, 0, 0, 1, 0),
                 (2, 1, 0, 0, 1), (2, 0, 0, 0, 1), (2, 1, 0, 2, 1))


def primary_form_of(form, opts):
    """The primary form of a query in trace form `form`."""
    return "none" if form == "per_pixel" else "resident" if form == "resident" else "per_lane"


def option_kw(opts):
    """The options of one parameter of the masked-call tests: an OPTION_TUPLES entry, "pool0" or "cast"."""
    if opts == "pool0":
        return {"pool": 0}
    if opts == "cast":
        return {}
    return dict(zip(("variant", "resident", "profile", "overlap", "primary_pooled"), opts))
