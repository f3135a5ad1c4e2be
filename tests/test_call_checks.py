"""csrc/sq_call_checks.h: the one "no two of these device buffers may overlap" check of the three libraries, as a stand-alone host
program (tests/call_checks_main.cpp) under AddressSanitizer and UndefinedBehaviorSanitizer.  No GPU, no library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NOTE = " (only d_out == d_color and d_out_var == d_var may share memory)"
WANT = [
    "touching: 0 ",
    "one byte: 1 a and b overlap",
    "inside: 1 big and small overlap",
    "null: 0 ",
    "both aliases: 0 ",
    "aliases not allowed: 1 d_color and d_out overlap",
    "shifted alias: 1 d_color and d_out overlap" + NOTE,
    "wrong pair: 1 d_color and d_out_var overlap" + NOTE,
    "no variance: 0 ",
    "pair test: 0 ",
]


def test_overlap_check_under_sanitizers(tmp_path):
    exe = str(tmp_path / "call_checks_main")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                           os.path.join(ROOT, "tests", "call_checks_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True)
    assert r.returncode == 0 and r.stderr == b"", (r.returncode, r.stderr[-2000:])
    assert r.stdout.decode().splitlines() == WANT
