"""bench.py's pure helpers (no GPU): the class-priced VALU figure, the staleness check of counter files, the build id, the output dump."""
import importlib
import importlib.util
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("sq_bench", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_valu_mix_weighted_is_the_priced_sum_over_simd_cycles():
    b = _bench()
    p = {"SQ_INSTS_VALU": 1000.0, "SQ_INSTS_VALU_ADD_F32": 200.0, "SQ_INSTS_VALU_MUL_F32": 100.0, "SQ_INSTS_VALU_FMA_F32": 50.0,
         "SQ_INSTS_VALU_TRANS_F32": 10.0, "SQ_INSTS_VALU_INT32": 140.0}
    secs = 1e-9
    m = b.valu_mix_weighted(p, secs)
    other = 1000 - 500
    base = 200 * b.VALU_PRICE["ADD_F32"] + 100 * b.VALU_PRICE["MUL_F32"] + 50 * b.VALU_PRICE["FMA_F32"] + 10 * b.VALU_PRICE["TRANS_F32"] + 140 * b.VALU_PRICE["INT32"]
    cyc = b.N_SIMD * b.CLOCK_HZ * secs
    assert abs(m["value"] - (base + other * b.VALU_PRICE_OTHER[1]) / cyc) < 1e-3
    assert m["low"] <= m["value"] <= m["high"] and m["unclassed_share"] == 0.5 and m["fp32_add_mul_fma_share"] == 0.35
    assert b.valu_mix_weighted({"SQ_INSTS_VALU": 5.0}, 1.0) is None and b.valu_mix_weighted(None, 1.0) is None
    # the committed counter file prices the headline kernel between its bounds
    prof = b.load_profile("latest_pmc.json")
    if prof and "SQ_INSTS_VALU_ADD_F32" in prof:
        m = b.valu_mix_weighted(prof, 0.043)
        assert 0.4 < m["low"] < m["value"] < m["high"] < 1.3


def test_counter_files_are_tied_to_a_build():
    b = _bench()
    assert b.stale_note(None, "x") is not None
    assert b.stale_note({"build_id": "abc"}, "abc") is None
    why = b.stale_note({"build_id": "abc"}, "def")
    assert "abc" in why and "def" in why
    assert "build_id" not in {} and b.stale_note({}, "def") is not None            # a file from before the stamp is stale by definition
    for name in ("latest_pmc.json", "latest_other_configs.json"):
        prof = json.load(open(os.path.join(ROOT, "profiles", name)))
        assert re.fullmatch(r"[0-9a-f]{16}", prof["build_id"]), name


def test_build_id_is_the_hash_of_the_sources_and_is_in_the_library():
    sqt = importlib.import_module("squigly-trace_amd")
    spec = importlib.util.spec_from_file_location("sq_build", os.path.join(ROOT, "squigly-trace_amd", "build.py"))
    bm = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bm)
    assert sqt.build_id() == bm.source_id() and not bm.stale()                     # the in-tree library is built from the sources that are here
    assert bm.source_id(("-DX=1",)) != bm.source_id()                              # a variant build has another identity


def test_dump_frame_writes_the_frame_as_float32_within_the_budget(tmp_path):
    """--dump-outputs: a frame that fits is written whole; a larger one as the same seeded sample of its pixels in every run."""
    import numpy as np
    import torch
    b = _bench()
    g = np.random.default_rng(7)
    small = torch.from_numpy(g.integers(0, 256, (40, 72, 3), dtype=np.uint8))
    b.dump_frame(str(tmp_path), small)
    got = np.load(tmp_path / "frame_rgb8.npy")
    assert got.dtype == np.float32 and np.array_equal(got, small.numpy().astype(np.float32))
    assert not (tmp_path / "frame_rgb8_pixels.npy").exists()
    big = torch.from_numpy(g.integers(0, 256, (2400, 2400, 3), dtype=np.uint8))    # 69 MB as float32
    for d in ("a", "b"):
        b.dump_frame(str(tmp_path / d), big)
    rgb, pix = np.load(tmp_path / "a" / "frame_rgb8.npy"), np.load(tmp_path / "a" / "frame_rgb8_pixels.npy")
    assert rgb.dtype == np.float32 and pix.dtype == np.float64
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64 << 20
    assert np.array_equal(rgb, big.numpy().reshape(-1, 3)[pix.astype(np.int64)].astype(np.float32))
    assert np.array_equal(pix, np.load(tmp_path / "b" / "frame_rgb8_pixels.npy"))
    assert len(np.unique(pix)) == len(pix) == b.DUMP_SAMPLE_PIXELS
    b.dump_frame(str(tmp_path / "a"), small)                                         # a smaller frame into the same directory
    assert not (tmp_path / "a" / "frame_rgb8_pixels.npy").exists()
