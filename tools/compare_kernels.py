#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds by instruction stream and resource figures.  CPU only.

    python tools/compare_kernels.py A B [--arch gfx950] [--objdump PATH]

A and B are libraries (or any file with embedded clang offload bundles) or bare AMDGPU code objects.  The code objects of the
architecture are taken out of each, disassembled with the ROCm tree's llvm-objdump, and every kernel's instruction text (comments
and addresses stripped) is hashed together with its resource figures from the code object's metadata (llvm-readelf --notes:
VGPRs, AGPRs, SGPRs, spills, static LDS, scratch, kernel-argument bytes, workgroup size, dynamic stack).  The two sides are then
matched as multisets of hashes, so a kernel that was only renamed counts as present in both.  Printed: the kernel counts, then every kernel without a counterpart with its instruction count.
Exit status 0 when every kernel of either side has a counterpart, 1 otherwise.
"""
import argparse
import collections
import hashlib
import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile

BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
PADDING = ("s_nop 0", "s_code_end", "...")       # behind a kernel's last instruction ("..." is the disassembler's run of zeros)


def find_tool(names, given=None):
    if given:
        return given
    roots = [os.environ.get("ROCM_PATH"), "/opt/rocm"]
    hipcc = shutil.which("hipcc")
    if hipcc:
        roots.append(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))))
    for name in names:
        for root in roots:
            for sub in ("llvm/bin", "lib/llvm/bin", "bin"):
                p = os.path.join(root, sub, name) if root else None
                if p and os.path.exists(p):
                    return p
        if shutil.which(name):
            return shutil.which(name)
    return None


def code_objects(path, arch):
    """The code objects for `arch` in the file: itself if it is a bare ELF for the GPU, otherwise every matching bundle entry."""
    with open(path, "rb") as f:
        data = f.read()
    if data[:4] == b"\x7fELF" and struct.unpack_from("<H", data, 18)[0] == 224:      # EM_AMDGPU
        return [data]
    if b"CCOB" in data and BUNDLE_MAGIC not in data:
        raise SystemExit("%s: compressed offload bundles are not supported (build with --no-offload-compress)" % path)
    out = []
    at = data.find(BUNDLE_MAGIC)
    while at >= 0:
        n, = struct.unpack_from("<Q", data, at + len(BUNDLE_MAGIC))
        p = at + len(BUNDLE_MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", data, p)
            triple = data[p + 24:p + 24 + tlen].decode()
            p += 24 + tlen
            if triple.startswith("hip") and triple.split("-")[-1].split(":")[0] == arch and size:
                out.append(data[at + off:at + off + size])
        at = data.find(BUNDLE_MAGIC, p)
    if not out:
        raise SystemExit("%s: no %s code object found" % (path, arch))
    return out


RESOURCES = ("agpr_count", "group_segment_fixed_size", "kernarg_segment_size", "max_flat_workgroup_size", "private_segment_fixed_size",
             "sgpr_count", "sgpr_spill_count", "uses_dynamic_stack", "vgpr_count", "vgpr_spill_count")


def resources_of(notes):
    """{mangled kernel name: "figure=value ..."} from the text of llvm-readelf --notes (one block per kernel, keys in order)."""
    out, cur = {}, {}
    for line in notes.splitlines():
        m = re.match(r"^\s+(?:- )?\.([a-z_]+):\s+(\S+)\s*$", line)
        if not m:
            continue
        key, val = m.groups()
        if key == "agpr_count":                    # the first key of a kernel's block
            cur = {}
        if key in RESOURCES or key == "name":      # (an argument's .name comes before the kernel's own and is overwritten by it)
            cur[key] = val
        if key == "vgpr_spill_count":              # the last figure of a block
            out[cur["name"]] = " ".join("%s=%s" % (k, cur.get(k, "?")) for k in RESOURCES)
    return out


def kernels_of(obj, objdump):
    """{mangled kernel name: [resource figures, instruction lines...]} of one code object."""
    with tempfile.NamedTemporaryFile(suffix=".co") as tmp:
        tmp.write(obj)
        tmp.flush()
        readelf = os.path.join(os.path.dirname(objdump), "llvm-readelf")
        figures = resources_of(subprocess.run([readelf, "--notes", tmp.name], check=True, capture_output=True, text=True).stdout)
        syms = subprocess.run([objdump, "-t", tmp.name], check=True, capture_output=True, text=True).stdout
        text = subprocess.run([objdump, "-d", "--no-show-raw-insn", "--no-leading-addr", tmp.name], check=True, capture_output=True, text=True).stdout
    is_kernel = {l.split()[-1][:-3] for l in syms.splitlines() if l.rstrip().endswith(".kd")}     # a kernel has a descriptor NAME.kd
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^(?:[0-9a-f]+ )?<([^>]+)>:\s*$", line)
        if m:
            cur = out.setdefault(m.group(1), []) if m.group(1) in is_kernel else None
            continue
        if cur is None:
            continue
        ins = re.sub(r"\s+", " ", line.split("//")[0]).strip()
        if ins:
            cur.append(re.sub(r"<[^>]*>", "<>", ins))      # a symbolised branch target carries the kernel's own name
    for ins in out.values():                               # what fills the gap up to the next symbol's alignment is no part of the kernel
        while ins and ins[-1] in PADDING:
            ins.pop()
    for name, ins in out.items():
        if name not in figures:
            raise SystemExit("no resource figures for kernel %s" % name)
        ins.insert(0, figures[name])
    return out


def load(path, arch, objdump):
    """[(name, hash, instruction count)] over every code object of the file."""
    out = []
    for obj in code_objects(path, arch):
        for name, ins in kernels_of(obj, objdump).items():
            out.append((name, hashlib.sha256("\n".join(ins).encode()).hexdigest(), len(ins) - 1))
    return out


def demangler():
    tool = find_tool(["llvm-cxxfilt", "c++filt"])
    def run(names):
        if not tool or not names:
            return {n: n for n in names}
        res = subprocess.run([tool], input="\n".join(names) + "\n", capture_output=True, text=True)
        lines = res.stdout.splitlines()
        return dict(zip(names, lines)) if res.returncode == 0 and len(lines) == len(names) else {n: n for n in names}
    return run


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--arch", default="gfx950")
    ap.add_argument("--objdump", default=None, help="llvm-objdump to use (default: the ROCm tree's)")
    args = ap.parse_args()
    objdump = find_tool(["llvm-objdump"], args.objdump)
    if not objdump:
        raise SystemExit("llvm-objdump not found")
    A, B = load(args.a, args.arch, objdump), load(args.b, args.arch, objdump)
    left = collections.Counter(h for _, h, _ in B)
    only_a, both = [], 0
    for k in A:
        if left[k[1]] > 0:
            left[k[1]] -= 1
            both += 1
        else:
            only_a.append(k)
    only_b = []
    for k in reversed(B):                      # what is left of B's multiset, one entry per unmatched copy
        if left[k[1]] > 0:
            left[k[1]] -= 1
            only_b.append(k)
    only_b.reverse()
    names = demangler()([k[0] for k in only_a + only_b])
    print("A: %s: %d kernels" % (args.a, len(A)))
    print("B: %s: %d kernels" % (args.b, len(B)))
    print("in both, by instruction stream and resource figures: %d" % both)
    for tag, ks in (("only in A", only_a), ("only in B", only_b)):
        print("%s: %d" % (tag, len(ks)))
        for name, _, n in sorted(ks, key=lambda k: names[k[0]]):
            print("  %6d instructions  %s" % (n, names[name]))
    return 1 if only_a or only_b else 0


if __name__ == "__main__":
    sys.exit(main())
