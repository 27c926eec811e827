"""Is the scorer's device code the same as another tree's?  For changes that only move source.

    python scripts/isa_same_as.py --parent DIR [--defines EWK_TIMING ...]

Compiles csrc/ewk_mfcc.hip of this tree and of the tree at DIR to gfx950 assembly with build.py's
flags (no GPU needed), blanks the __hip_cuid_<hash> symbol hipcc derives from the file, and
compares the two texts.  Prints `identical`, or the first function that differs, and exits 1.
"""
from __future__ import annotations

import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from easywakeword_amd import build as B  # noqa: E402

SRC = "ewk_mfcc.hip"


def asm(root, defines, out):
    cmd = [B._hipcc(), f"--offload-arch={B.ARCH}", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function"] + \
        B.EXTRA.get(SRC, []) + [f"-D{d}" for d in defines] + \
        ["--cuda-device-only", "-S", os.path.join(root, "easywakeword_amd", "csrc", SRC), "-o", out]
    subprocess.run(cmd, check=True)
    return re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_", open(out).read()).split("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="root of the tree to compare with")
    ap.add_argument("--defines", nargs="*", default=[])
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        new = asm(ROOT, args.defines, os.path.join(tmp, "new.s"))
        old = asm(os.path.abspath(args.parent), args.defines, os.path.join(tmp, "old.s"))
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
