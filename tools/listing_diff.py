#!/usr/bin/env python3
"""Device listings of csrc/*.hip at a parent revision against this tree: the proof a refactor carries that the kernels
are unchanged.  Every file is compiled with build.py's FLAGS + FILE_FLAGS plus `-S --offload-device-only`, once in a
`git worktree` of the parent and once here; the listings are compared line by line, ignoring `.file` / `.ident` lines and
the path-hashed `__hip_cuid_` symbol.  Needs hipcc only, no GPU.

    tools/listing_diff.py [--rev HEAD] [--work DIR] [--jobs N] [--by-kernel] [inst_german.hip ...]

DIR (default: a fresh temporary directory) keeps the worktree and both sets of listings; the parent's are reused when
they are already there.  Exit status 1 if any listing differs.

--by-kernel is for a change that removes (or adds) kernels: that renumbers the local labels of every function behind
them and reorders the metadata, so no line-by-line comparison can show the survivors unchanged.  Each listing is cut into
its functions, the bodies and the kernel descriptors are compared by mangled name (by_kernel below), and per file the
kernels only in the parent, only in this tree, and differing are named.  Exit status 1 if any differs or is new."""
import argparse
import concurrent.futures
import importlib.util
import os
import re
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


_FUNC_TYPE = re.compile(r"\s*\.type\s+([^,\s]+),@function")
_FUNC_END = re.compile(r"\.Lfunc_end\d+:")
_PER_FUNC = re.compile(r"\.L(BB|JTI|CPI|func_begin|func_end)\d+")      # .LBB<function index>_<block> and kin
_PER_FILE = re.compile(r"\.L(?:tmp|post_getpc)\d+")                   # numbered through the whole file


def cut_functions(text):
    """{mangled name: (body, descriptor)} of a device listing.  A body is the lines from the function's label to its
    `.Lfunc_end`, comments and the descriptor aside, with the function's index in its local labels replaced by `#` and
    the file-wide `.Ltmp` labels numbered from 0 in order of appearance; a kernel's descriptor is its `.amdhsa_*` lines
    (registers, LDS, scratch), empty for a plain device function."""
    out, functions, name = {}, set(), None
    for ln in text.splitlines():
        m = _FUNC_TYPE.match(ln)
        if m:
            functions.add(m.group(1))
        if name is None:
            label = ln.split(":", 1)[0]
            if ":" in ln and label in functions:
                name, body, desc, seen, in_desc = label, [], [], {}, False
            continue
        if _FUNC_END.match(ln):
            out[name] = (tuple(body), tuple(desc))
            name = None
            continue
        ln = ln.split(";", 1)[0].rstrip()
        if ln.lstrip().startswith(".amdhsa_kernel"):
            in_desc = True
        elif ln.lstrip().startswith(".end_amdhsa_kernel"):
            in_desc = False
        elif in_desc:
            desc.append(ln.strip())
        elif ln:
            ln = _PER_FUNC.sub(lambda m: ".L%s#" % m.group(1), ln)
            body.append(_PER_FILE.sub(lambda m: ".Ltmp#%d" % seen.setdefault(m.group(0), len(seen)), ln))
    return out


def by_kernel(parent_text, this_text):
    """(only in the parent, only in this tree, body or descriptor differs, equal): sorted lists of mangled names."""
    p, t = cut_functions(parent_text), cut_functions(this_text)
    both = sorted(set(p) & set(t))
    return (sorted(set(p) - set(t)), sorted(set(t) - set(p)),
            [k for k in both if p[k] != t[k]], [k for k in both if p[k] == t[k]])


def _report_by_kernel(f, parent_s, this_s):
    with open(parent_s) as fp, open(this_s) as ft:
        gone, new, differ, equal = by_kernel(fp.read(), ft.read())
    print("%-28s %4d equal  %d differ  %d only in parent  %d only in this tree" % (f, len(equal), len(differ), len(gone), len(new)))
    for tag, names in (("differs", differ), ("only in parent", gone), ("only in this tree", new)):
        for k in names:
            print("    %-18s %s" % (tag, k))
    return len(differ) + len(new)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rev", default="HEAD")
    ap.add_argument("--work", default=None)
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--by-kernel", action="store_true")
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
        if a.by_kernel:
            bad += _report_by_kernel(f, *(os.path.join(work, side, f[:-4] + ".s") for side in ("parent", "this"))) != 0
            continue
        p, t = (_lines(os.path.join(work, side, f[:-4] + ".s")) for side in ("parent", "this"))
        n = sum(x != y for x, y in zip(p, t)) + abs(len(p) - len(t))
        print("%-28s %7d lines  %d differ" % (f, len(t), n))
        bad += n != 0
    print("listings in %s" % work)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
