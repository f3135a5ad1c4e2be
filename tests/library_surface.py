"""What the test modules of the seven shared libraries hold a library's surface to, written once: the functions its header declares
against the Python list and the dynamic symbol table, whether it is a client of the main library, and its build id among the seven
of squigly-trace_amd/build.py's table LIBS.  Belongs here: those checks and the readers under them; no test, and nothing of one
library alone -- the expected symbol sets, salts, macros and link lines stay in the library's own test module."""
import importlib.util
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_module():
    """squigly-trace_amd/build.py as a module of the caller's own: a test may point its CSRC at a copy of the tree."""
    spec = importlib.util.spec_from_file_location("sq_build_for_a_library_test", os.path.join(ROOT, "squigly-trace_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def files(b, *names):
    """The sources and headers of the named rows of b.LIBS, as one list."""
    return [f for n in names for f in b.LIBS[n]["sources"] + b.LIBS[n]["headers"]]


def declared_in(header, prefix):
    """The functions with `prefix` that include/<header> declares (comments aside)."""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(%s[a-z0-9_]+)\s*\(" % prefix, text))


def exported_by(path):
    """The sq_ functions in the dynamic symbol table of the library at `path`."""
    nm = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
    return set(re.findall(r" T (sq_[a-z0-9_]+)", nm))


def check_exports(mod, headers, prefix, exact=True):
    """What the headers declare is mod.EXPORTED_SYMBOLS and is what the library exports -- exact: and nothing else, so that nothing
    of another library's leaks out of this one -- and every declared function can be looked up.  Returns the declared set."""
    declared = set().union(*(declared_in(h, prefix) for h in ([headers] if isinstance(headers, str) else headers)))
    assert declared == set(mod.EXPORTED_SYMBOLS), declared ^ set(mod.EXPORTED_SYMBOLS)
    exported = exported_by(mod.LIB_PATH)
    assert declared <= exported, declared - exported
    assert not exact or exported <= declared, exported - declared
    for name in declared:
        assert getattr(mod.lib(), name) is not None
    return declared


def check_client(path, client, never=()):
    """client: the library needs libsquigly_hip.so and finds it beside itself; otherwise it needs nothing of it.  never: names of
    libraries it must not need either way."""
    needed = subprocess.check_output(["readelf", "-d", path]).decode()
    if client:
        assert "libsquigly_hip.so" in needed and "$ORIGIN" in needed
    else:
        assert "libsquigly_hip" not in needed
    for other in never:
        assert other not in needed, other


def check_ids(b, name, mod, sqt, tmp_path, edits):
    """The ids of b.LIBS are distinct; the loaded library `mod` and the main library carry theirs, and the in-tree product is not
    stale; a copy of the tree elsewhere keeps every id; and appending to a file -- edits: (file, the rows that list it and so must
    move) in turn -- moves those ids and no other."""
    ids = lambda: {n: b.lib_source_id(lib) for n, lib in b.LIBS.items()}                          # noqa: E731
    before = ids()
    assert len(set(before.values())) == len(b.LIBS)
    assert mod.build_id() == before[name] and sqt.build_id() == before["main"] == b.source_id()
    assert not b.lib_stale(b.LIBS[name]) and not b.stale()
    shutil.copytree(os.path.join(ROOT, "squigly-trace_amd", "csrc"), tmp_path / "a" / "b" / "csrc")
    shutil.copytree(os.path.join(ROOT, "include"), tmp_path / "a" / "include")
    b.CSRC = str(tmp_path / "a" / "b" / "csrc")
    assert ids() == before
    for file, moves in edits:
        assert set(moves) == {n for n in b.LIBS if file in files(b, n)}, file
        with open(os.path.join(b.CSRC, file), "a") as fh:
            fh.write("// changed\n")
        after = ids()
        assert {n for n in after if after[n] != before[n]} == set(moves), file
        before = after
    return before
