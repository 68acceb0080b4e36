#!/usr/bin/env python3
"""Compare the gfx950 device assembly of .hip files between two source trees or git revisions.

    tools/device_asm_diff.py OLD NEW k_screen_bf16.hip [more.hip ...]

OLD / NEW: a directory holding a source tree, or a git revision of this repository (written out with
`git archive` into a temporary directory).  Each file is compiled with the flags its own tree's
vq_amd/csrc/Makefile uses (read from `make -n`) plus `--cuda-device-only -S`; the `__hip_cuid_<hash>`
symbol, which hashes the source text, is replaced by a fixed token, and the two texts are compared kernel
by kernel.  Identical text is identical instructions, register counts, LDS and scratch: a refactor that
passes changes neither what a kernel computes nor how fast.  Exit status 1 if any kernel (or the rest of
the file: the metadata behind the kernels) differs.  Needs hipcc and no GPU; ~40 s per file and side.
"""
import argparse
import os
import re
import shlex
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("vq_amd", "csrc")
BEGIN = re.compile(r"; -- Begin function (\S+)")
REST = "(rest of the file)"


def materialise(spec, tmp, tag):
    """A directory as it is; anything else is a git revision, exported under tmp."""
    if os.path.isdir(spec):
        return os.path.abspath(spec)
    rev = subprocess.run(["git", "-C", REPO, "rev-parse", "--verify", spec + "^{commit}"], check=True,
                         stdout=subprocess.PIPE, text=True).stdout.strip()
    out = os.path.join(tmp, tag)
    os.mkdir(out)
    tar = os.path.join(tmp, tag + ".tar")
    subprocess.run(["git", "-C", REPO, "archive", "-o", tar, rev], check=True)
    subprocess.run(["tar", "-xf", tar, "-C", out], check=True)
    return out


def compile_command(tree, name):
    """The Makefile's own command for the file's object, minus `-c SRC -o OBJ`."""
    obj = os.path.splitext(name)[0] + ".o"
    lines = subprocess.run(["make", "-n", "-W", name, obj], cwd=os.path.join(tree, CSRC), check=True,
                           stdout=subprocess.PIPE, text=True).stdout.splitlines()
    for line in lines:
        words = shlex.split(line)
        if "-c" in words and name in words:
            drop = {words.index("-c"), words.index(name)}
            if "-o" in words:
                drop |= {words.index("-o"), words.index("-o") + 1}
            return [w for i, w in enumerate(words) if i not in drop]
    raise SystemExit(f"{tree}: make -n shows no compile command for {name}")


def device_asm(tree, name, out):
    cmd = compile_command(tree, name) + ["--cuda-device-only", "-S", name, "-o", out]
    p = subprocess.run(cmd, cwd=os.path.join(tree, CSRC), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)} failed in {tree}:\n{p.stdout}")
    with open(out) as f:
        return re.sub(r"__hip_cuid_[0-9a-f]{16}", "__hip_cuid_X", f.read())


def split_kernels(text):
    """{kernel: its text, REST: everything in front of the first and behind the last kernel}.  A kernel's text
    runs from its `Begin function` line to the next one; behind the last kernel it ends at the first section
    that is neither code, kernel descriptor nor the kernel's resource summary."""
    parts, rest, name = {}, [], None
    for line in text.splitlines(keepends=True):
        m = BEGIN.search(line)
        if m:
            name = m.group(1)
            parts[name] = []
        elif name and line.startswith("\t.section") and not re.match(r"\t\.section\t\.(text|rodata|AMDGPU\.csdata)", line):
            name = None
        (parts[name] if name else rest).append(line)
    out = {k: "".join(v) for k, v in parts.items()}
    out[REST] = "".join(rest)
    return out


def demangle(names):
    tool = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not tool:
        return {n: n for n in names}
    res = subprocess.run([tool], input="\n".join(names), stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()
    return dict(zip(names, res))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("old", help="source tree (directory) or git revision")
    ap.add_argument("new", help="source tree (directory) or git revision")
    ap.add_argument("files", nargs="+", help=".hip file names under vq_amd/csrc")
    args = ap.parse_args()
    differ = 0
    with tempfile.TemporaryDirectory() as tmp:
        trees = [materialise(args.old, tmp, "old"), materialise(args.new, tmp, "new")]
        for name in args.files:
            with ThreadPoolExecutor(2) as ex:
                old, new = ex.map(lambda i: split_kernels(device_asm(trees[i], name, os.path.join(tmp, f"{i}.s"))), (0, 1))
            kernels = [k for k in old if k != REST] + [k for k in new if k not in old]
            pretty = demangle(kernels)
            print(f"== {name}: {args.old} -> {args.new}")
            bad = 0
            for k in kernels + [REST]:
                verdict = "identical" if old.get(k) == new.get(k) else "only in OLD" if k not in new else \
                    "only in NEW" if k not in old else "DIFFERS"
                bad += verdict != "identical"
                print(f"{verdict:11s} {pretty.get(k, k)}")
            print(f"== {name}: {len(kernels)} kernels, {bad} not identical")
            differ += bad
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
