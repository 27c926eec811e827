"""Is a source's device code the same as another tree's?  For changes that only move source.

    python scripts/isa_same_as.py --parent DIR [--src ewk_gate.hip] [--by-function] [--defines EWK_TIMING ...]

Compiles csrc/<src> (default ewk_mfcc.hip) of this tree and of the tree at DIR to gfx950 assembly
with build.py's flags (no GPU needed), blanks the __hip_cuid_<hash> symbol hipcc derives from the
file, and compares the two texts.  Prints `identical`, or the first function that differs, and
exits 1.  DIR may also be an assembly file kept from an earlier run (--keep FILE writes this
tree's).

--by-function is for changes that rename or renumber symbols (a lambda inside a kernel is part of
the mangled name of every helper instantiated on it) but must leave the instructions alone: the
text is split at function labels, comments go, every function symbol becomes a name that does not
depend on the mangling (k_gate_ticks<RB,DMA,PROF,LSN>, a kernel's plain name, helpers by position),
every other symbol and local label the order of its first appearance in the function, and each
function -- instructions, its .amdhsa_ block and its metadata entry (register counts, scratch,
LDS, kernarg size) -- is reported as `same` or with its first differing line.
"""
from __future__ import annotations

import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from easywakeword_amd import build as B  # noqa: E402


def asm(root, src, defines, out):
    if os.path.isfile(root):
        out = root
    else:
        cmd = [B._hipcc(), f"--offload-arch={B.ARCH}", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function"] + \
            B.EXTRA.get(src, []) + [f"-D{d}" for d in defines] + \
            ["--cuda-device-only", "-S", os.path.join(root, "easywakeword_amd", "csrc", src), "-o", out]
        subprocess.run(cmd, check=True)
    return re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_", open(out).read()).split("\n")


LABEL = re.compile(r"^([A-Za-z_][\w$]*):")
SYMBOL = re.compile(r"_Z\w+|\.L\w+")
GATE = re.compile(r"_ZN3ewk12k_gate_ticksILi(\d+)ELi(\d+)ELb([01])ELb([01])EEEvNS_8GateArgsE$")


def functions(lines):
    """[(name, lines)] per function, mangling-free (see the module comment)."""
    meta = lines.index("amdhsa.kernels:") if "amdhsa.kernels:" in lines else len(lines)
    chunks = []   # [symbol, lines]
    for l in lines[:meta]:
        m = LABEL.match(l)
        if m:
            chunks.append([m.group(1), []])
        l = l.split(";")[0].rstrip()
        if chunks and l.strip():
            chunks[-1][1].append(l)
    entries, by_symbol = [], {c[0]: c for c in chunks}   # a kernel's metadata entry goes behind its function
    for l in lines[meta + 1:]:
        if l.startswith("amdhsa.target"):
            break
        if l.startswith("  - "):
            entries.append([])
        entries[-1].append(l)
    for e in entries:
        sym = next(m.group(1) for l in e for m in [re.match(r"\s+\.name:\s+(\S+)", l)] if m)
        by_symbol[sym][1] += ["(metadata)"] + e
    names, helpers = {}, 0
    for sym, _ in chunks:
        g = GATE.match(sym)
        n = re.match(r"_ZN3ewk(\d+)", sym)
        plain = sym[len(n.group(0)):][:int(n.group(1))] if n else sym
        if g:
            names[sym] = "k_gate_ticks<%s,%s,%s,%s>" % g.groups()
        elif plain.startswith("k_") or not n:
            names[sym] = plain
        else:
            helpers += 1
            names[sym] = f"helper {helpers} ({plain})"
    out = []
    for sym, body in chunks:
        local = {}
        sub = lambda m: names.get(m.group(0)) or local.setdefault(m.group(0), f"<{len(local) + 1}>")  # noqa: E731
        out.append((names[sym], [SYMBOL.sub(sub, l) for l in body]))
    return out


def by_function(new, old):
    new, old = functions(new), dict(functions(old))
    bad = 0
    for name, body in new:
        ref = old.pop(name, None)
        if ref == body:
            print(f"same     {name}  ({len(body)} lines)")
            continue
        bad += 1
        if ref is None:
            print(f"new      {name}")
            continue
        k = next((i for i, (a, b) in enumerate(zip(body, ref)) if a != b), min(len(body), len(ref)))
        print(f"DIFFERS  {name}  at line {k + 1} of {len(body)} / {len(ref)}\n    this tree: "
              f"{body[k].strip() if k < len(body) else '<end>'}\n    parent:    {ref[k].strip() if k < len(ref) else '<end>'}")
    for name in old:
        bad += 1
        print(f"gone     {name}")
    print(f"{len(new) - bad + len(old)} of {len(new) + len(old)} functions same" if bad else f"all {len(new)} functions same")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="root of the tree to compare with, or its kept assembly")
    ap.add_argument("--src", default="ewk_mfcc.hip")
    ap.add_argument("--by-function", action="store_true")
    ap.add_argument("--keep", help="write this tree's assembly here as well")
    ap.add_argument("--defines", nargs="*", default=[])
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        new = asm(ROOT, args.src, args.defines, os.path.join(tmp, "new.s"))
        if args.keep:
            shutil.copy(os.path.join(tmp, "new.s"), args.keep)
        old = asm(os.path.abspath(args.parent), args.src, args.defines, os.path.join(tmp, "old.s"))
    if args.by_function:
        return by_function(new, old)
    if new == old:
        print("identical")
        return 0
    k = next((i for i, (a, b) in enumerate(zip(new, old)) if a != b), min(len(new), len(old)))
    func = next((m.group(1) for l in reversed(new[:k + 1]) for m in [re.match(r"^(\w+):", l)] if m), "(before any function)")
    print(f"differs: line {k + 1}, in {func}\n  this tree: {new[k] if k < len(new) else '<end>'}\n"
          f"  parent:    {old[k] if k < len(old) else '<end>'}")
    return 1


if __name__ == "__main__":
    sys.exit(main())
