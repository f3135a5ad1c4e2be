"""CPU tests of the progressive-rendering surface: the range entry point of the C-ABI, the CLI flag and the argument checks
of the Python layer that come before any device work (the renders themselves: tests/test_gpu_progressive.py)."""
import os
import re
import subprocess

import pytest

from conftest import ROOT


def _declarations():
    text = open(os.path.join(ROOT, "include", "squigly_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_the_range_entry_point_and_the_library_exports_it(sqt):
    decl = re.search(r"int\s+sq_render_rows_device_range\s*\(([^)]*)\)\s*;", _declarations())
    assert decl, "sq_render_rows_device_range is not declared in include/squigly_hip.h"
    params = [p.split()[-1].lstrip("*") for p in decl.group(1).split(",")]
    assert params == ["s", "cam", "samples", "w", "h", "cast", "sh", "k_begin", "k_end", "d_sum", "d_avg", "d_rgb", "hip_stream"]
    assert "sq_render_rows_device_range" in sqt.EXPORTED_SYMBOLS
    nm = subprocess.check_output(["nm", "-D", "--defined-only", sqt.LIB_PATH]).decode()
    assert re.search(r" T sq_render_rows_device_range$", nm, flags=re.M)
    L = sqt.lib()
    assert len(L.sq_render_rows_device_range.argtypes) == 13
    assert L.sq_abi_version() == 1                                   # an addition: the ABI stays compatible


def test_cli_accepts_preview_every_and_defaults_to_no_previews():
    from importlib import import_module
    cli = import_module("squigly-trace_amd.cli")
    p = cli.build_parser()
    assert p.parse_args([]).preview_every is None
    assert p.parse_args(["--preview-every", "3"]).preview_every == 3
    for bad in ("0", "-2", "x"):
        with pytest.raises(SystemExit):
            p.parse_args(["--preview-every", bad])


def test_render_progressive_is_exported_and_checks_its_step(sqt):
    gen = sqt.render_progressive(None, None, 4, (8, 8), 0)
    with pytest.raises(ValueError):
        next(gen)                                                     # refused before a scene is uploaded


def test_progressive_checks_its_counts_before_touching_a_device(sqt):
    for samples, done in ((0, 0), (4, -1), (4, 5)):
        with pytest.raises(ValueError):
            sqt.Progressive(None, None, samples, 8, 8, done=done)
