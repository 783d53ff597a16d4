#!/usr/bin/env python3
"""Device listings of csrc/*.hip at a parent revision against this tree: the proof a refactor carries that the kernels
are unchanged.  Every file is compiled with build.py's FLAGS + FILE_FLAGS plus `-S --offload-device-only`, once in a
`git worktree` of the parent and once here; the listings are compared line by line, ignoring `.file` / `.ident` lines and
the path-hashed `__hip_cuid_` symbol.  Needs hipcc only, no GPU.

    tools/listing_diff.py [--rev HEAD] [--work DIR] [--jobs N] [inst_german.hip ...]

DIR (default: a fresh temporary directory) keeps the worktree and both sets of listings; the parent's are reused when
they are already there.  Exit status 1 if any listing differs."""
import argparse
import concurrent.futures
import importlib.util
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = os.path.join("autoreparam_amd", "csrc")


def _build_py():
    spec = importlib.util.spec_from_file_location("arp_build_py", os.path.join(ROOT, "autoreparam_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _listing(hipcc, flags, src, out):
    r = subprocess.run([hipcc] + flags + ["-S", "--offload-device-only", src, "-o", out],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed on %s:\n%s" % (src, r.stdout))


def _lines(path):
    with open(path) as f:
        return [ln for ln in f if ".file" not in ln and ".ident" not in ln and "__hip_cuid_" not in ln]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rev", default="HEAD")
    ap.add_argument("--work", default=None)
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("files", nargs="*")
    a = ap.parse_args()
    b = _build_py()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    work = os.path.abspath(a.work or tempfile.mkdtemp(prefix="listing_diff_"))
    tree = os.path.join(work, "tree")
    if not os.path.isdir(tree):
        subprocess.run(["git", "-C", ROOT, "worktree", "add", "--detach", tree, a.rev], check=True)
    files = a.files or sorted(f for f in os.listdir(os.path.join(ROOT, REL)) if f.endswith(".hip"))
    jobs = []
    for side, top in (("parent", tree), ("this", ROOT)):
        os.makedirs(os.path.join(work, side), exist_ok=True)
        for f in files:
            out = os.path.join(work, side, f[:-4] + ".s")
            if side == "this" or not os.path.exists(out):
                jobs.append((hipcc, b.FLAGS + b.FILE_FLAGS.get(f, []), os.path.join(top, REL, f), out))
    with concurrent.futures.ThreadPoolExecutor(max_workers=a.jobs) as ex:
        list(ex.map(lambda j: _listing(*j), jobs))
    bad = 0
    for f in files:
        p, t = (_lines(os.path.join(work, side, f[:-4] + ".s")) for side in ("parent", "this"))
        n = sum(x != y for x, y in zip(p, t)) + abs(len(p) - len(t))
        print("%-28s %7d lines  %d differ" % (f, len(t), n))
        bad += n != 0
    print("listings in %s" % work)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
