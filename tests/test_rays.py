"""CPU tests of the ray-query surface: the two entry points of the C-ABI (sq_intersect_rays_device, sq_camera_rays_device), their
bindings, and the checks that come before any device work (the queries themselves: tests/test_gpu_rays.py)."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

DECLS = {
    "sq_intersect_rays_device": ["s", "d_org", "d_dir", "n", "d_tri", "d_dist", "d_point", "hip_stream"],
    "sq_camera_rays_device": ["s", "cam", "w", "h", "sh", "d_org", "d_dir", "hip_stream"],
}


def _declarations():
    text = open(os.path.join(ROOT, "include", "squigly_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


@pytest.mark.parametrize("name", sorted(DECLS))
def test_header_declares_the_query_entry_points_and_the_library_exports_them(sqt, name):
    decl = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", _declarations())
    assert decl, f"{name} is not declared in include/squigly_hip.h"
    params = [p.split()[-1].lstrip("*") for p in decl.group(1).split(",")]
    assert params == DECLS[name]
    assert name in sqt.EXPORTED_SYMBOLS
    nm = subprocess.check_output(["nm", "-D", "--defined-only", sqt.LIB_PATH]).decode()
    assert re.search(r" T " + name + "$", nm, flags=re.M)
    assert len(getattr(sqt.lib(), name).argtypes) == len(DECLS[name])


def test_abi_version_is_unchanged(sqt):
    assert sqt.lib().sq_abi_version() == 1                          # an addition: the ABI stays compatible


def test_c_calls_on_a_null_scene_are_refused_with_a_message(sqt):
    L = sqt.lib()
    buf = np.zeros(12, np.float32)
    tri = np.zeros(4, np.int32)
    for n in (4, -1, 0):
        assert L.sq_intersect_rays_device(None, buf.ctypes.data, buf.ctypes.data, n, tri.ctypes.data, None, None, None) != 0
        assert len(L.sq_last_error()) > 0
    cam = sqt.camera_from_text(open(os.path.join(ROOT, "data", "camera")).read().encode())
    assert L.sq_camera_rays_device(None, cam, 2, 2, sqt.Shard(2, 0, 1), buf.ctypes.data, buf.ctypes.data, None) != 0
    assert len(L.sq_last_error()) > 0


@pytest.mark.parametrize("o_shape, d_shape", [((4, 2), (4, 2)), ((4, 3), (5, 3)), ((3,), (4, 3)), ((2, 3, 3), (6, 3)), ((), ())])
def test_intersect_refuses_bad_shapes_before_any_device_work(sqt, o_shape, d_shape):
    from importlib import import_module
    device = import_module("squigly-trace_amd.device")
    with pytest.raises(sqt.SquiglyError):
        device.DeviceScene.intersect(None, np.zeros(o_shape, np.float32), np.zeros(d_shape, np.float32))   # no scene: the check comes first


def test_hits_is_a_named_triple(sqt):
    h = sqt.Hits(1, 2, 3)
    assert (h.tri, h.dist, h.point) == (1, 2, 3)
