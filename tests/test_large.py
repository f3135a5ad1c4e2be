"""CPU tests of the frame-size limits: the row-shard arithmetic at widths up to 2^31 - 1, and the Python layer's
refusal of frames that are too large for one call, which comes before any allocation or device work and carries the library's
own words (the library's refusals themselves, and the frames just inside them: tests/test_gpu_large.py)."""
import ctypes as C
import os

import pytest

from conftest import ROOT

CAMERA = open(os.path.join(ROOT, "data", "camera")).read()
INT32_MAX = 2 ** 31 - 1


def py_shard_rows(w, rb, si, ns):
    """sq_shard_rows in Python integers: the rows of the blocks si, si + ns, ... of ceil(w / rb) blocks of rb rows."""
    nblocks = (w + rb - 1) // rb
    mine = len(range(si, nblocks, ns))
    if mine == 0:
        return 0
    last_block = si + (mine - 1) * ns
    return (mine - 1) * rb + (min((last_block + 1) * rb, w) - last_block * rb)


def py_global_row(j, rb, si, ns):
    blk = j // rb
    return (blk * ns + si) * rb + (j - blk * rb)


@pytest.mark.parametrize("w", [46341, INT32_MAX])
@pytest.mark.parametrize("rb", [2, 8])
@pytest.mark.parametrize("ns", [1, 3, 8])
def test_shard_rows_and_global_row_at_large_widths(sqt, w, rb, ns):
    """The row counts of the shards sum to w, and a shard's first and last local rows, and the local rows on both sides of every
    block boundary near them, map to the global rows Python integers give.  sq_shard_global_row multiplies in int32_t: for a local
    row j < sq_shard_rows(w, sh) every intermediate is at most the global row itself, which is below w <= 2^31 - 1."""
    L = sqt.lib()
    total = 0
    for si in range(ns):
        sh = sqt.Shard(rb, si, ns)
        rows = L.sq_shard_rows(w, sh)
        assert rows == py_shard_rows(w, rb, si, ns), (w, rb, si, ns)
        total += rows
        probes = {j for j in (0, 1, rb - 1, rb, rb + 1, rows // 2, rows - rb - 1, rows - rb, rows - 2, rows - 1) if 0 <= j < rows}
        for j in sorted(probes):
            g = L.sq_shard_global_row(j, sh)
            assert g == py_global_row(j, rb, si, ns), (w, rb, si, ns, j)
            assert 0 <= g < w and (g // rb) % ns == si
    assert total == w


def test_python_shard_rows_match_the_c_functions_at_46341(sqt):
    L = sqt.lib()
    w = 46341
    for rb in (2, 8):
        for ns in (1, 3, 8):
            seen = 0
            for si in range(ns):
                sh = sqt.Shard(rb, si, ns)
                rows = sqt.dist.shard_rows(w, rb, si, ns)
                assert len(rows) == L.sq_shard_rows(w, sh)
                for j in (0, 1, rb, len(rows) // 2, len(rows) - 2, len(rows) - 1):
                    assert rows[j] == L.sq_shard_global_row(j, sh), (rb, ns, si, j)
                seen += len(rows)
            assert seen == w


def test_frame_size_error_states_the_limits_from_both_sides(sqt):
    f = sqt.frame_size_error
    assert sqt.MAX_CALL_PIXELS == INT32_MAX and sqt.MAX_WAVEFRONT_PIXELS == 2 ** 29
    assert f(46340, 46340) is None                                   # 2 147 395 600 <= 2^31 - 1
    assert f(1, INT32_MAX) is None and f(INT32_MAX, 1) is None
    assert f(46341, 46341) == "46341 x 46341 pixels exceed 2^31 - 1 pixels in one call"
    assert f(2, 2 ** 30) == f"2 x {2 ** 30} pixels exceed 2^31 - 1 pixels in one call"
    assert f(INT32_MAX, INT32_MAX, 7).startswith(f"7 views of {INT32_MAX} x {INT32_MAX} pixels exceed 2^31 - 1")
    assert f(3, 715827883, 1) is not None and f(715827882, 3, 1) is None
    assert f(16, 12, (2 ** 31 - 1) // (16 * 12) + 1) is not None and f(16, 12, (2 ** 31 - 1) // (16 * 12)) is None
    # the wavefront form: 2^29 pixels
    assert f(2 ** 14, 2 ** 15, wavefront=True) is None
    assert f(23171, 23173, wavefront=True) == ("23171 x 23173 pixels exceed 2^29 pixels in one call of the wavefront form "
                                               "(variant 1 and cast frames take 2^31 - 1)")
    assert f(23171, 23173, wavefront=False) is None
    assert f(2 ** 14, 2 ** 14, 3, wavefront=True) == (f"3 views of {2 ** 14} x {2 ** 14} pixels exceed 2^29 pixels in one call of the "
                                                      "wavefront form (variant 1 takes 2^31 - 1)")
    assert f(46341, 46341, wavefront=True) == f(46341, 46341)       # the larger limit is named first
    assert f(0, 5) is None and f(5, 0) is None


def _fake_scene(sqt, variant=None):
    """A DeviceScene that was never uploaded: every call on it that reaches the device or an allocation fails otherwise."""
    ds = object.__new__(sqt.DeviceScene)
    ds.device = 0
    ds._h = None
    if variant is not None:
        ds._variant = variant
    return ds


def test_python_layer_refuses_oversized_frames_before_allocating(sqt):
    """No GPU here: torch.empty(..., device="cuda") or the C call on a NULL scene would fail in its own way, so a SquiglyError
    with the size message shows that the check came first."""
    import torch
    cam = sqt.camera_from_text(CAMERA.encode())
    big = dict(w=46341, h=46341)
    ds = _fake_scene(sqt)
    msg = "46341 x 46341 pixels exceed 2^31 - 1 pixels in one call"
    sums = torch.empty((1, 1, 3))                                    # never looked at: the size check comes before the tensor checks
    calls = {
        "render_rows": lambda d: d.render_rows(cam, 1, cast=True, **big),
        "render_rows_range": lambda d: d.render_rows_range(cam, 1, big["w"], big["h"], 0, 1, sums, cast=True),
        "render_rows_masked": lambda d: d.render_rows_masked(cam, 1, big["w"], big["h"], 0, 1, sums, cast=True),
        "Progressive": lambda d: sqt.Progressive(d, cam, 1, cast=True, **big),
        "Adaptive": lambda d: sqt.Adaptive(d, cam, 1, tol=0.1, cast=True, **big),
    }
    for what, call in calls.items():
        for d in (ds, _fake_scene(sqt, variant=1)):
            with pytest.raises(sqt.SquiglyError) as e:
                call(d)
            assert str(e.value) == msg, what
    with pytest.raises(sqt.SquiglyError) as e:
        ds.render_views([cam, cam, cam], 1, 2 ** 15, 2 ** 15, cast=True)
    assert str(e.value) == f"3 views of {2 ** 15} x {2 ** 15} pixels exceed 2^31 - 1 pixels in one call"
    # one shard of two of the same frame is below the limit: the refusal is about the shard's pixels, not the frame's
    assert sqt.frame_size_error(sqt.lib().sq_shard_rows(46341, sqt.Shard(8, 0, 2)), 46341) is None
    # the wavefront form (the default; a fake scene never saw set_option) refuses above 2^29 pixels, the per-pixel forms do not
    wmsg = "23171 x 23173 pixels exceed 2^29 pixels in one call of the wavefront form (variant 1 and cast frames take 2^31 - 1)"
    for what, call in {"render_rows": lambda d, c: d.render_rows(cam, 1, 23171, 23173, cast=c),
                       "Progressive": lambda d, c: sqt.Progressive(d, cam, 1, 23171, 23173, cast=c),
                       "Adaptive": lambda d, c: sqt.Adaptive(d, cam, 1, 23171, 23173, tol=0.1, cast=c)}.items():
        with pytest.raises(sqt.SquiglyError) as e:
            call(ds, False)
        assert str(e.value) == wmsg, what
    for d, c in ((ds, True), (_fake_scene(sqt, variant=1), False)):
        with pytest.raises(Exception) as e:                          # accepted by the size check: fails later, for want of a GPU or a scene
            d.render_rows(cam, 1, 23171, 23173, cast=c, want_avg=False)
        assert "exceed" not in str(e.value)


def test_c_calls_on_a_null_scene_still_say_null_argument_first(sqt):
    L = sqt.lib()
    cam = sqt.camera_from_text(CAMERA.encode())
    sh = sqt.Shard(46341, 0, 1)
    assert L.sq_render_rows_device(None, C.byref(cam), 1, 46341, 46341, 1, sh, None, None, None) != 0
    assert L.sq_last_error() == b"null argument"
    assert L.sq_render_rows_device_masked(None, C.byref(cam), 1, 46341, 46341, 1, sh, 0, 1, None, C.c_void_p(256), None, None, None, None, None) != 0
    assert L.sq_last_error() == b"null argument"
    assert L.sq_camera_rays_device(None, C.byref(cam), 46341, 46341, sh, None, None, None) != 0
    assert L.sq_last_error() == b"null argument"
    assert L.sq_adaptive_update_device(None, 2 ** 32, None, None, None, 0.1, 1.0, None, None, None) != 0
    assert L.sq_last_error() == b"null argument"
    assert L.sq_abi_version() == 1
