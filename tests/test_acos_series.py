"""Host sq::facos (squigly-trace_amd/csrc/sq_math.h) against the oracle's sqo_acosf(., TRIG_CRD), bit for bit, on the arguments of
tests/acos_cases.py: crd::acos_ evaluates the arcsine series once for both of its ranges, and every value it returns must be the one
the oracle's two-armed form gives.  The host code is reached through a stand-alone program (tests/acos_main.cpp), compiled without
contraction as the library is."""
import os
import subprocess

import numpy as np

import acos_cases as AC
from conftest import ROOT


def test_arguments_cover_both_ranges_and_their_edges():
    x = AC.arguments()
    assert 290_000 <= len(x) <= 320_000
    a = np.abs(x[np.isfinite(x)])
    assert (a <= 0.5).sum() > 100_000 and ((a > 0.5) & (a <= 1)).sum() > 100_000 and (a > 1).sum() >= AC.ULPS
    for v in (0.5, -0.5, 1.0, -1.0):                                    # both neighbours of every edge
        assert (x == np.nextafter(np.float32(v), np.float32(9))).any() and (x == np.nextafter(np.float32(v), np.float32(-9))).any()
    assert np.isnan(x).sum() == 1 and np.isinf(x).sum() == 2 and (x.view(np.uint32) == 0x80000000).any()


def test_host_facos_equals_the_oracle_bit_for_bit(tmp_path):
    exe, fin, fout = str(tmp_path / "acos_main"), str(tmp_path / "in.f32"), str(tmp_path / "out.f32")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", os.path.join(ROOT, "tests", "acos_main.cpp"), "-o", exe])
    AC.arguments().tofile(fin)
    r = subprocess.run([exe, fin, fout], capture_output=True)
    assert r.returncode == 0 and r.stderr == b"", (r.returncode, r.stderr[-2000:])
    AC.assert_bit_equal(np.fromfile(fout, np.float32), "host sq::facos")
