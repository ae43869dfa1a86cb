#!/usr/bin/env python
"""Is the device code of a HIP source the same as at a git revision?  Both trees are compiled for gfx950 with the build's flags
(-S --cuda-device-only), comment lines, assembler directives and the __hip_cuid_ label are dropped, and the instruction streams are
compared per kernel symbol, whole.  Prints `same` or the two instruction counts for every kernel.
usage: python tools/isa_same.py <git-rev> point-of-interest-recommendation_amd/csrc/filter.hip ...
The revision's assembly is kept under $TMPDIR/isa_same/<commit>/ so that a second run compiles the working tree only."""
import concurrent.futures as cf
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S", "--cuda-device-only"]
run = lambda cmd, **kw: subprocess.run(cmd, check=True, capture_output=True, text=True, **kw).stdout


def assembly(root, rel, out):
    if not os.path.exists(out):
        subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + [os.path.join(root, rel), "-o", out + ".tmp"], check=True)
        os.replace(out + ".tmp", out)
    return out


def streams(path):
    """{symbol: [instruction or local label, ...]}; local labels keep their order, not the function's number in the file"""
    syms, cur, meta = {}, None, False
    for line in open(path):
        line = line.split(";", 1)[0].strip()
        if line.startswith(".amdgpu_metadata") or line.startswith(".end_amdgpu_metadata"):
            meta = line.startswith(".amdgpu_metadata")
        if not line or meta:
            continue
        m = re.match(r"([A-Za-z_$][\w.$]*):$", line)
        if m:
            cur = None if m.group(1).startswith("__hip_cuid_") else syms.setdefault(m.group(1), [])
        elif cur is not None and (not line.startswith(".") or line.endswith(":")):
            cur.append(re.sub(r"\.LBB\d+_", ".LBB_", " ".join(line.split())))
    return {k: v for k, v in syms.items() if v}


def main():
    rev, files = sys.argv[1], [os.path.relpath(os.path.abspath(f), ROOT) for f in sys.argv[2:]]
    sha = run(["git", "-C", ROOT, "rev-parse", rev + "^{commit}"]).strip()
    old = os.path.join(tempfile.gettempdir(), "isa_same", sha)
    if not os.path.isdir(os.path.join(old, "tree")):      # extracted under another name, then renamed: an interrupted run leaves no tree
        os.makedirs(old, exist_ok=True)
        part = tempfile.mkdtemp(prefix="tree.", dir=old)
        tar = subprocess.run(["git", "-C", ROOT, "archive", sha], check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", part], input=tar, check=True)
        os.rename(part, os.path.join(old, "tree"))
    name = lambda rel: os.path.basename(rel)[:-4] + ".s"
    with tempfile.TemporaryDirectory(prefix="isa_same_new_") as new, cf.ThreadPoolExecutor(min(16, 2 * len(files))) as ex:
        a = [ex.submit(assembly, os.path.join(old, "tree"), f, os.path.join(old, name(f))) for f in files]
        b = [ex.submit(assembly, ROOT, f, os.path.join(new, name(f))) for f in files]
        pairs = [(f, streams(x.result()), streams(y.result())) for f, x, y in zip(files, a, b)]
    syms = sorted({s for _, x, y in pairs for s in set(x) | set(y)})
    names = dict(zip(syms, run(["c++filt"] + syms).splitlines())) if syms else {}
    differ = 0
    for f, x, y in pairs:
        for sym in sorted(set(x) | set(y)):
            same = x.get(sym) == y.get(sym)
            differ += not same
            dem = re.sub(r"^void poi::", "", names[sym].strip())
            print("%-14s %-96s %s" % (os.path.basename(f), dem[:96], "same" if same else "%d / %d" % (len(x.get(sym, [])), len(y.get(sym, [])))))
    print("%d kernels differ" % differ)
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
