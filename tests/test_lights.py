"""CPU tests of the caller-given lights' surface: the two entry points of the C-ABI (sq_scene_set_lights, sq_scene_get_lights), their
bindings, DeviceScene.set_lights' checks that come before any device work, and the CLI's --light (the lights themselves:
tests/test_gpu_lights.py)."""
import os
import re
import subprocess
from importlib import import_module

import numpy as np
import pytest

from conftest import ROOT

DECLS = {
    "sq_scene_set_lights": ("int", ["s", "lights", "n_lights", "hip_stream"]),
    "sq_scene_get_lights": ("int32_t", ["s", "out", "cap"]),
}


def _declarations():
    text = open(os.path.join(ROOT, "include", "squigly_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


@pytest.mark.parametrize("name", sorted(DECLS))
def test_header_declares_the_light_entry_points_and_the_library_exports_them(sqt, name):
    ret, names = DECLS[name]
    decl = re.search(ret + r"\s+" + name + r"\s*\(([^)]*)\)\s*;", _declarations())
    assert decl, f"{name} is not declared in include/squigly_hip.h"
    assert [p.split()[-1].lstrip("*") for p in decl.group(1).split(",")] == names
    assert name in sqt.EXPORTED_SYMBOLS
    nm = subprocess.check_output(["nm", "-D", "--defined-only", sqt.LIB_PATH]).decode()
    assert re.search(r" T " + name + "$", nm, flags=re.M)
    assert len(getattr(sqt.lib(), name).argtypes) == len(names)


def test_sq_light_is_six_floats_and_the_abi_version_is_unchanged(sqt):
    import ctypes as C
    assert re.search(r"typedef\s+struct\s*\{\s*float\s+pos\[3\];\s*float\s+power\[3\];\s*\}\s*sq_light;", _declarations())
    assert C.sizeof(sqt._native.Light) == 24
    assert sqt.lib().sq_abi_version() == 1
    assert re.search(r"#define\s+SQ_ABI_VERSION\s+1\b", open(os.path.join(ROOT, "include", "squigly_hip.h")).read())
    assert sqt.REFERENCE_LIGHT == ((0.0, 3.0, -1.0), (2.0, 2.0, 2.0)) and sqt.MAX_LIGHTS == 4096


def test_c_calls_on_a_null_scene_are_refused_with_a_message(sqt):
    L = sqt.lib()
    lights = (sqt._native.Light * 2)()
    out = np.full(12, 7.5, np.float32)
    for arr, n in ((lights, 2), (None, 0), (lights, -1)):
        assert L.sq_scene_set_lights(None, arr, n, None) != 0
        assert len(L.sq_last_error()) > 0
    assert L.sq_scene_get_lights(None, out.ctypes.data, 2) == -1
    assert len(L.sq_last_error()) > 0 and (out == 7.5).all()


class _NoDevice:
    """Stands in for a DeviceScene: any use of the device or the handle is an AttributeError, not a SquiglyError."""


@pytest.mark.parametrize("bad", [
    [], np.zeros((0, 6), np.float32), np.zeros((3, 5), np.float32), np.zeros((3, 7), np.float32), np.zeros(6, np.float32),
    np.zeros((4097, 6), np.float32), [((0, 0), 2.0)], [((0, 0, 0), (1, 2))], [((0, 0, 0), (1, 2, 3, 4))], [((0, 0, 0),)], 5, "light",
], ids=lambda b: type(b).__name__ + (str(getattr(b, "shape", "")) if hasattr(b, "shape") else str(b)[:24]))
def test_set_lights_refuses_bad_shapes_and_counts_before_any_device_work(sqt, bad):
    with pytest.raises(sqt.SquiglyError):
        import_module("squigly-trace_amd.device").DeviceScene.set_lights(_NoDevice(), bad)


def test_light_tables_from_every_spelling(sqt):
    A = sqt._native.lights_array
    want = np.array([[0, 3, -1, 2, 2, 2], [1, 2, 3, 4, 5, 6]], np.float32)
    for spelling in (want, want.tolist(), [((0, 3, -1), 2), ((1, 2, 3), (4, 5, 6))], [sqt.REFERENCE_LIGHT, (np.array([1, 2, 3]), [4.0, 5.0, 6.0])]):
        got = A(spelling)
        assert got.dtype == np.float32 and got.flags["C_CONTIGUOUS"] and np.array_equal(got, want)
    assert A(np.zeros((4096, 6))).shape == (4096, 6)


def test_cli_parses_lights_in_order_and_refuses_them_without_cast(sqt, capsys):
    cli = import_module("squigly-trace_amd.cli")
    a = cli.parse_args(["--cast", "--light", "1,2,3", "--light", "0,-1.5,2,0.5", "--light", "(4,5,6,0.1,0.2,0.3)"])
    assert a.light == [((1.0, 2.0, 3.0), (2.0, 2.0, 2.0)), ((0.0, -1.5, 2.0), (0.5, 0.5, 0.5)), ((4.0, 5.0, 6.0), (0.1, 0.2, 0.3))]
    assert np.array_equal(sqt._native.lights_array(a.light), np.array([[1, 2, 3, 2, 2, 2], [0, -1.5, 2, .5, .5, .5], [4, 5, 6, .1, .2, .3]], np.float32))
    # a value that starts with '-' is taken for an option unless it is attached with '=' or parenthesised
    b = cli.parse_args(["--cast", "--light=-1,2,3", "--light", "(-0.5,-2,3,4)"])
    assert b.light == [((-1.0, 2.0, 3.0), (2.0, 2.0, 2.0)), ((-0.5, -2.0, 3.0), (4.0, 4.0, 4.0))]
    with pytest.raises(SystemExit):
        cli.parse_args(["--cast", "--light", "-1,2,3"])
    assert "--light=" in cli.build_parser().format_help()
    assert cli.parse_args(["--cast"]).light is None
    for argv in (["--light", "1,2,3"], ["--cast", "--light", "1,2"], ["--cast", "--light", "1,2,3,4,5"], ["--cast", "--light", "a,b,c"]):
        with pytest.raises(SystemExit):
            cli.parse_args(argv)
    assert "--light" in capsys.readouterr().err
