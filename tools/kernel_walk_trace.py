#!/usr/bin/env python3
"""Proves which kernels the kernel walk (tests/kernel_walk.py) launches, and records it in tests/golden/kernel_walk.json:

    python tools/kernel_walk_trace.py --commit <hash of the commit the library was built from> [--out FILE] [--dir TRACE_DIR]

Needs a GPU.  Runs `python tests/kernel_walk.py` once under `rocprofv3 --kernel-trace --mangled-kernels` (no other tracing, no counters;
one process under one time limit), reads the trace CSV and cuts it into per-case segments at the walk's markers: before case i the
walk issues a debug_eval of one element, the only one-workgroup launches of sq_debug_kernel in the run.  The file holds the commit, the
library's build id, the command, and for every kernel of the library's gfx950 code objects (ELF symbol table: the NAME.kd descriptors)
its mangled name, its short demangled spelling (kernel_walk.short_name) and the cases in whose segment it was dispatched; the kernels
of kernel_walk.UNREACHABLE are listed apart.

Exit status 1 when a case failed, a kernel a case claims is missing from its segment, or the launched kernels plus UNREACHABLE are
not exactly the library's kernels.  Kernels a case launched without claiming them are reported only.

    python tools/kernel_walk_trace.py --unlaunched-by -- python -m pytest tests -q -m gpu

traces any other command the same way and prints the library's kernels it never dispatched (nothing is written)."""
import argparse
import csv
import glob
import importlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
import compare_kernels as CK  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "kernel_walk.json")
ARCH = "gfx950"
MARKER = "sq_debug_kernel"


def kernel_symbols(path):
    """The mangled names of the kernels in the library's gfx950 code objects, sorted, from their symbol tables alone."""
    readelf = CK.find_tool(["llvm-readelf"])
    if not readelf:
        raise SystemExit("llvm-readelf not found")
    names = set()
    for obj in CK.code_objects(path, ARCH):
        with tempfile.NamedTemporaryFile(suffix=".co") as tmp:
            tmp.write(obj)
            tmp.flush()
            table = subprocess.run([readelf, "--symbols", "--wide", tmp.name], check=True, capture_output=True, text=True).stdout
        for line in table.splitlines():
            f = line.split()
            if len(f) >= 8 and f[3] == "OBJECT" and f[-1].endswith(".kd"):       # a kernel has a descriptor NAME.kd
                names.add(f[-1][:-3])
    return sorted(names)


def library_kernels(path):
    """{mangled name: short demangled name} of the library's kernels."""
    import kernel_walk as KW
    names = kernel_symbols(path)
    demangled = CK.demangler()(names)
    if any(demangled[n] == n for n in names if n.startswith("_Z")):
        raise SystemExit("no working demangler (llvm-cxxfilt or c++filt)")
    return {n: KW.short_name(demangled[n]) for n in names}


def trace(command, out_dir, limit):
    """Runs the command under the kernel trace; returns (exit status, [(kernel name, workgroups or work-items of the grid)] in start order)."""
    full = ["timeout", "-k", "10", str(limit), "rocprofv3", "--kernel-trace", "--mangled-kernels", "--output-format", "csv", "-d", out_dir, "--"] + command
    rc = subprocess.run(full, cwd=ROOT).returncode
    rows = []
    for path in glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                name = r["Kernel_Name"]
                name = name[:-3] if name.endswith(".kd") else name
                grid = r.get("Grid_Size", r.get("Grid_Size_X", "0"))
                rows.append((int(r["Start_Timestamp"]), name, int(grid)))
    rows.sort()
    return rc, [(n, g) for _, n, g in rows], full


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--commit", help="the commit the loaded library was built from")
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--dir", default=None, help="where the trace is written (default: a temporary directory)")
    ap.add_argument("--timeout", type=int, default=900, help="seconds the traced process may take")
    ap.add_argument("--unlaunched-by", action="store_true", help="trace the command after -- and print the kernels it never dispatched")
    ap.add_argument("command", nargs="*")
    args = ap.parse_args()
    sqt = importlib.import_module("squigly-trace_amd")                 # importing the package loads no library
    kernels = library_kernels(sqt.LIB_PATH)
    out_dir = args.dir or tempfile.mkdtemp(prefix="kernel_walk_")
    os.makedirs(out_dir, exist_ok=True)
    if args.unlaunched_by:
        rc, rows, full = trace(args.command, out_dir, args.timeout)
        seen = {n for n, _ in rows}
        missing = sorted(kernels[m] for m in kernels if m not in seen)
        print(f"exit status {rc}; {len(kernels) - len(missing)} of {len(kernels)} kernels dispatched; never dispatched: {len(missing)}")
        for name in missing:
            print("  " + name)
        with open(os.path.join(out_dir, "dispatched.json"), "w") as f:   # for the union over several commands
            json.dump({"exit_status": rc, "dispatched": sorted(kernels[m] for m in kernels if m in seen)}, f, indent=1)
        return 0
    if not args.commit:
        raise SystemExit("--commit is required")
    import kernel_walk as KW
    result_path = os.path.join(out_dir, "walk.json")
    rc, rows, full = trace([sys.executable, os.path.join("tests", "kernel_walk.py"), result_path], out_dir, args.timeout)
    if not os.path.exists(result_path):
        raise SystemExit(f"the walk wrote no result (exit status {rc})")
    with open(result_path) as f:
        walk = json.load(f)
    failed = {k: v for k, v in walk["results"].items() if v != "passed"}
    marker = [m for m, s in kernels.items() if s == MARKER]
    assert len(marker) == 1, marker
    segments, cur = [], None
    for name, grid in rows:
        if name == marker[0] and grid in (1, 256):                     # a marker: exactly one workgroup (as workgroups or as work-items)
            cur = set()
            segments.append(cur)
        if cur is not None and name in kernels:
            cur.add(name)
    bad = []
    if len(segments) != len(KW.CASES) or walk["cases"] != KW.NAMES:
        bad.append(f"{len(segments)} markers in the trace for {len(KW.CASES)} cases")
    by_short = {s: m for m, s in kernels.items()}
    launched = {m: [] for m in kernels}
    for c, seg in zip(KW.CASES, segments):
        for m in sorted(seg):
            launched[m].append(c.name)
        missing = [k for k in c.claims if by_short.get(k) not in seg]
        if missing:
            bad.append(f"{c.name}: claimed but not dispatched: {missing}")
        extra = sorted(kernels[m] for m in seg if kernels[m] not in c.claims and kernels[m] != MARKER)
        if extra:
            print(f"{c.name}: also dispatched {extra}")
    unreachable = sorted(m for m, s in kernels.items() if s in KW.UNREACHABLE)
    if len(unreachable) != len(KW.UNREACHABLE):
        bad.append("a kernel of UNREACHABLE is not in the library")
    never = sorted(kernels[m] for m in kernels if not launched[m] and m not in unreachable)
    both = sorted(kernels[m] for m in unreachable if launched[m])
    if never:
        bad.append(f"neither launched nor unreachable: {never}")
    if both:
        bad.append(f"listed unreachable, yet launched: {both}")
    for k, v in failed.items():
        bad.append(f"{k} failed: {v}")
    n_launched = sum(1 for m in kernels if launched[m])
    print(f"{len(kernels)} kernels: {n_launched} launched by {len(segments)} cases, {len(unreachable)} unreachable")
    for line in bad:
        print("ERROR: " + line)
    if bad:
        return 1
    shown = " ".join("python" if a == sys.executable else a for a in full).replace(out_dir, "DIR")
    head = {"commit": args.commit, "library": walk["build_id"], "command": shown, "n_cu": walk["n_cu"], "n_cases": len(KW.CASES)}
    with open(args.out, "w") as f:
        f.write("{\n" + ",\n".join(f' "{k}": {json.dumps(v)}' for k, v in head.items()) + ',\n "kernels": [\n')
        f.write(",\n".join("  " + json.dumps({"mangled": m, "name": kernels[m], "cases": launched[m]}) for m in kernels if launched[m]))
        f.write('\n ],\n "unreachable": [\n')
        f.write(",\n".join("  " + json.dumps({"mangled": m, "name": kernels[m]}) for m in unreachable))
        f.write("\n ]\n}\n")
    print(f"-> {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
