"""CPU tests of the multi-view surface: the views entry point of the C-ABI, the CLI flag --views and its file format, and the
argument checks of the Python layer that come before any device work (the renders themselves: tests/test_gpu_views.py)."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT

CAMERA = open(os.path.join(ROOT, "data", "camera")).read()


def _declarations():
    text = open(os.path.join(ROOT, "include", "squigly_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _cli():
    from importlib import import_module
    return import_module("squigly-trace_amd.cli")


def test_header_declares_the_views_entry_point_and_the_library_exports_it(sqt):
    decl = re.search(r"int\s+sq_render_views_device\s*\(([^)]*)\)\s*;", _declarations())
    assert decl, "sq_render_views_device is not declared in include/squigly_hip.h"
    params = [p.split()[-1].lstrip("*") for p in decl.group(1).split(",")]
    assert params == ["s", "cams", "n_views", "samples", "w", "h", "cast", "sh", "k_begin", "k_end", "d_sum", "d_avg", "d_rgb",
                      "hip_stream"]
    assert "sq_render_views_device" in sqt.EXPORTED_SYMBOLS
    nm = subprocess.check_output(["nm", "-D", "--defined-only", sqt.LIB_PATH]).decode()
    assert re.search(r" T sq_render_views_device$", nm, flags=re.M)
    assert len(sqt.lib().sq_render_views_device.argtypes) == 14


def test_abi_version_is_unchanged(sqt):
    assert sqt.lib().sq_abi_version() == 1                          # an addition: the ABI stays compatible


def test_views_file_parser_accepts_pairs_of_camera_lines(sqt):
    cli = _cli()
    one = sqt.camera_from_text(CAMERA.encode())
    cams = cli.parse_views(CAMERA + "\n\n" + CAMERA + "  \n0.5 6 1\n1.4 0.15 0.2\n")
    assert len(cams) == 3
    for c in cams[:2]:
        assert list(c.pos) == list(one.pos) and list(c.rot) == list(one.rot)
    want = sqt.camera_from_text(b"0.5 6 1\n1.4 0.15 0.2\n")
    assert list(cams[2].pos) == list(want.pos) and list(cams[2].rot) == list(want.rot)


@pytest.mark.parametrize("text", ["", "\n \n", "0 7 0.75\n", CAMERA + "0 7 0.75\n", "0 7\n1 0 0\n", "0 7 0.75 1\n1 0 0\n",
                                  "0 7 x\n1 0 0\n", "0 7 0.75\n1 0 0\n0 1 2\n"])
def test_views_file_parser_refuses_odd_unparsable_and_empty_files(text):
    with pytest.raises(ValueError):
        _cli().parse_views(text)


def test_cli_parses_views_and_refuses_bad_files_and_previews(tmp_path):
    cli = _cli()
    assert cli.parse_args([]).views is None
    good = tmp_path / "views"
    good.write_text(CAMERA * 2)
    assert len(cli.parse_args(["--views", str(good)]).views) == 2
    assert cli.view_paths("render/result.png", 2) == ["render/result_0000.png", "render/result_0001.png"]
    odd, bad, empty = tmp_path / "odd", tmp_path / "bad", tmp_path / "empty"
    odd.write_text(CAMERA + "1 2 3\n")
    bad.write_text("0 7 0.75\nnot numbers here\n")
    empty.write_text("\n")
    for argv in (["--views", str(odd)], ["--views", str(bad)], ["--views", str(empty)], ["--views", str(tmp_path / "missing")],
                 ["--views", str(good), "--preview-every", "2"]):
        with pytest.raises(SystemExit):
            cli.parse_args(argv)


def test_render_views_refuse_an_empty_camera_list_before_any_device_work(sqt):
    with pytest.raises(ValueError):
        sqt.DeviceScene.render_views(None, [], 4, 8, 8)             # no scene: the check comes first
    with pytest.raises(ValueError):
        sqt.render_views_rgb8(None, [], 4, (8, 8))                  # refused before a scene is uploaded


def test_c_call_on_a_null_scene_is_refused_with_a_message(sqt):
    L = sqt.lib()
    cam = sqt.camera_from_text(CAMERA.encode())
    rc = L.sq_render_views_device(None, C.byref(cam), 1, 4, 8, 8, 0, sqt.Shard(8, 0, 1), 0, 4, None, None, None, None)
    assert rc != 0
    assert len(L.sq_last_error()) > 0
