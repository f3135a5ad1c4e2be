"""The reference-side binding (integration/LibHip.hs + integration/reference.patch) checked by inspection, mechanically.

No GHC exists here, so the shim cannot be compiled.  What CAN be checked: that reference.patch applies to the
reference as it is, and that every name LibHip.hs and DumpGolden.hs import from a reference module is in that module's
export list once the patch is applied (the shim named constructors src/BIH.hs does not export).

The reference's sources are not part of this repository.  tests/golden/reference_modules.json records what these
checks need from them: the export list of every module under src/ before and after the patch, and the SHA-256 of the
lines each hunk of the patch replaces, as the reference holds them.  Regenerate it from a checkout of the reference:

    python tests/test_integration_shim.py <reference checkout>
"""
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATCH = os.path.join(ROOT, "integration", "reference.patch")
FIXTURE = os.path.join(ROOT, "tests", "golden", "reference_modules.json")


def exports_of(text):
    """Names in a module's export list ('Name' and 'Type(..)' both as 'Name'); None = no list, everything is exported."""
    text = re.sub(r"\{-.*?-\}", "", text, flags=re.S)
    text = re.sub(r"--.*", "", text)
    m = re.search(r"\bmodule\s+[\w.]+\s*(\((.*?)\))?\s*where", text, flags=re.S)
    assert m, text[:200]
    if m.group(1) is None:
        return None
    body = re.sub(r"\(\.\.\)", "", m.group(2))
    return {n.strip() for n in body.split(",") if n.strip()}


def imports_of(path):
    """[(module, [names])] for every `import M (a, B (..), c)` with an explicit list."""
    text = open(path).read()
    text = re.sub(r"--.*", "", text)
    out = []
    for m in re.finditer(r"^import\s+(?:qualified\s+)?([\w.]+)(?:\s+as\s+\w+)?\s*\(((?:[^()]|\([^()]*\))*)\)", text, flags=re.M):
        names = [re.sub(r"\s*\(.*\)\s*$", "", n).strip() for n in re.split(r",(?![^()]*\))", m.group(2))]
        out.append((m.group(1), [n for n in names if n]))
    return out


def hunks_of(path):
    """[(file, old_start, old_lines, new_lines)] of a unified diff; the line lists hold bytes without their newline.
    Asserts that every hunk's body has exactly the line counts its header states."""
    out, cur, target = [], None, None
    for line in open(path, "rb").read().split(b"\n"):
        if line.startswith(b"+++ "):
            target = line[4:].split(b"\t")[0].decode().split("/", 1)[1]
            continue
        if line.startswith(b"--- ") or line.startswith(b"diff "):
            continue
        m = re.match(rb"^@@ -(\d+),(\d+) \+(\d+),(\d+) @@", line)
        if m:
            cur = (target, int(m.group(1)), [], [], int(m.group(2)), int(m.group(4)))
            out.append(cur)
            continue
        if cur is None or not line:
            continue
        tag, body = line[:1], line[1:]
        if tag in (b" ", b"-"):
            cur[2].append(body)
        if tag in (b" ", b"+"):
            cur[3].append(body)
    for f, start, old, new, n_old, n_new in out:
        assert (len(old), len(new)) == (n_old, n_new), f"{f} @@ -{start}: body has {len(old)} / {len(new)} lines, header says {n_old} / {n_new}"
    return [(f, start, old, new) for f, start, old, new, _, _ in out]


def lines_sha256(lines):
    return hashlib.sha256(b"\n".join(lines)).hexdigest()


def names_added_by_patch(rel):
    """Export-list names on the patch's '+' lines for one file, minus those on its '-' lines."""
    plus, minus, target = set(), set(), None
    for line in open(PATCH).read().splitlines():
        if line.startswith("+++ "):
            target = line[4:].split("\t")[0].split("/", 1)[1]
            continue
        if line.startswith("--- ") or target != rel:
            continue
        if line[:1] in ("+", "-"):
            names = {re.sub(r"\(\.\.\)", "", n).strip(" (") for n in line[1:].split(",")}
            (plus if line[0] == "+" else minus).update(n for n in names if re.fullmatch(r"[A-Za-z_][\w']*", n))
    return plus - minus


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_patch_applies_and_is_three_small_hunks(recorded):
    text = open(PATCH).read()
    files = re.findall(r"^\+\+\+ b/(\S+)", text, flags=re.M)
    assert sorted(files) == ["app/Main.hs", "squigly-trace.cabal", "src/BIH.hs"]
    added = [l for l in text.splitlines() if l.startswith("+") and not l.startswith("+++")]
    removed = [l for l in text.splitlines() if l.startswith("-") and not l.startswith("---")]
    assert len(added) <= 10 and len(removed) <= 3          # "what a maintainer changes" stays a handful of lines
    # it applies: every hunk's context and removed lines are, byte for byte, the reference's lines at the stated position
    hunks = hunks_of(PATCH)
    assert sorted(f"{f}:{s}" for f, s, _, _ in hunks) == sorted(recorded["patch_preimage_sha256"])
    for f, start, old, _ in hunks:
        assert lines_sha256(old) == recorded["patch_preimage_sha256"][f"{f}:{start}"], f"hunk {f} @@ -{start} no longer matches the reference"
    new = {f: b"\n".join(n).decode() for f, _, _, n in hunks}
    assert "renderHip scene cam settings" in new["app/Main.hs"]
    assert "LibHip" in new["squigly-trace.cabal"]


def test_recorded_exports_are_the_patch_applied():
    """The patched export lists of the fixture are the unpatched ones plus exactly what the patch adds to src/<M>.hs."""
    mods = json.load(open(FIXTURE))["modules"]
    assert set(mods) >= {"BIH", "Geometry", "Lib", "Obj"}
    for name, m in mods.items():
        if m["exports"] is None:
            assert m["exports_patched"] is None, name
            continue
        assert set(m["exports_patched"]) == set(m["exports"]) | names_added_by_patch(f"src/{name}.hs"), name


@pytest.mark.parametrize("shim", ["LibHip.hs", "DumpGolden.hs"])
def test_every_name_imported_from_the_reference_is_exported(recorded, shim):
    mods = recorded["modules"]
    checked = 0
    for module, names in imports_of(os.path.join(ROOT, "integration", shim)):
        if module not in mods:
            continue
        exp = mods[module]["exports_patched"]
        if exp is None:
            continue                                        # e.g. V3: no export list
        for n in names:
            assert n in exp, f"{shim}: `{n}` is not exported by {module} ({sorted(exp)})"
            checked += 1
    assert checked >= 5


def test_unpatched_bih_lacks_the_constructors_the_patch_adds(recorded):
    """The reason for hunk 1: without it LibHip.hs cannot see Leaf / Branch / BIHN."""
    exp = set(recorded["modules"]["BIH"]["exports"])
    assert not ({"Tree", "BIHNode", "BIHTree"} & exp)


def test_shim_uses_the_extensions_and_imports_it_needs():
    text = open(os.path.join(ROOT, "integration", "LibHip.hs")).read()
    assert "RecordWildCards" in text and "Settings {..}" in text             # src/Lib.hs:13 enables it for the same pattern
    assert "ForeignFunctionInterface" in text
    assert re.search(r"import qualified Graphics\.ColorSpace\s+as M", text)   # Pixel / RGB / PixelRGB, as src/Lib.hs:39-40
    assert "M.PixelRGB" in text and "M.Pixel M.RGB Word8" in text
    # sq_scene offsets used by the pokes = the C header's layout
    hdr = open(os.path.join(ROOT, "include", "squigly_hip.h")).read()
    assert re.search(r"sq_bounds\s+root;.*const sq_node\*\s+nodes;\s+int32_t n_nodes;.*const sq_tri\*\s+tris;\s+int32_t n_tris;.*"
                     r"const sq_material\*\s+mats;\s+int32_t n_mats;.*int32_t\s+height;", hdr, flags=re.S)
    # ... and the ctypes mirror of the same struct agrees on every offset the shim pokes at (x86-64)
    import ctypes
    import importlib
    nat = importlib.import_module("squigly-trace_amd._native")
    S = nat.Scene
    assert (S.nodes.offset, S.n_nodes.offset, S.tris.offset, S.n_tris.offset, S.mats.offset, S.n_mats.offset, S.height.offset,
            ctypes.sizeof(S), ctypes.sizeof(nat.Camera)) == (24, 32, 40, 48, 56, 64, 68, 72, 48)
    for off in ("pScene 24", "pScene 32", "pScene 40", "pScene 48", "pScene 56", "pScene 64", "pScene 68"):
        assert off in text


def record(ref):
    """Write FIXTURE from a checkout of the reference: export lists before and after `patch -p1`, hunk pre-image hashes."""
    def module_exports(tree):
        src = os.path.join(tree, "src")
        return {os.path.splitext(f)[0]: exports_of(open(os.path.join(src, f)).read())
                for f in sorted(os.listdir(src)) if f.endswith(".hs")}
    sha = {}
    for f, start, old, _ in hunks_of(PATCH):
        lines = open(os.path.join(ref, f), "rb").read().split(b"\n")
        assert lines[start - 1:start - 1 + len(old)] == old, f"{f} @@ -{start}: the patch does not apply to {ref}"
        sha[f"{f}:{start}"] = lines_sha256(old)
    with tempfile.TemporaryDirectory() as d:
        for rel in ("src", "app", "squigly-trace.cabal"):
            (shutil.copytree if os.path.isdir(os.path.join(ref, rel)) else shutil.copy)(os.path.join(ref, rel), os.path.join(d, rel))
        subprocess.run(["patch", "-p1", "--batch", "--quiet", "-i", PATCH], cwd=d, check=True)
        patched = module_exports(d)
    before = module_exports(ref)
    out = {"what": "export lists of the reference's src/ modules before and after integration/reference.patch, and the SHA-256 "
                   "of the reference's lines that each hunk (file:first line) replaces; written by tests/test_integration_shim.py",
           "modules": {m: {"exports": None if e is None else sorted(e),
                           "exports_patched": None if patched[m] is None else sorted(patched[m])} for m, e in before.items()},
           "patch_preimage_sha256": sha}
    with open(FIXTURE, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", FIXTURE)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: python tests/test_integration_shim.py <reference checkout>")
    record(sys.argv[1])
