#!/usr/bin/env python3
"""Build one library per seeded fault:  python tools/mutants_build.py [-j N] [name ...]   (no name: every tools/mutants/*.diff)

Per diff: csrc/ and include/ are copied to variants/src_<name>/, the diff is applied there, the objects whose sources include
the touched file are recompiled with the Makefile's compiler and flags, and variants/lib_<name>.so is linked from them and the
unmodified objects of `make -C socialways_amd/csrc` (run first if they are missing or stale).  Needs no GPU.  Select a
library with SW_LIB_PATH=variants/lib_<name>.so (socialways_amd/_lib.py), or hand the names to tools/mutants_run.py."""
import argparse
import concurrent.futures
import glob
import os
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("socialways_amd", "csrc")
MUTANTS = os.path.join(ROOT, "tools", "mutants")


def makefile_vars():
    text = open(os.path.join(ROOT, CSRC, "Makefile")).read()
    var = {}
    for name in ("HIPCC", "ARCH", "FLAGS", "SRCS"):
        m = re.search(r"^%s\s*\??=\s*(.*)$" % name, text, re.M)
        if not m:
            sys.exit("no %s line in %s/Makefile" % (name, CSRC))
        var[name] = m.group(1).strip()
    var["FLAGS"] = var["FLAGS"].replace("$(ARCH)", var["ARCH"])
    return var


def touched_file(diff):
    """The one file under csrc/ a diff changes (its '+++ b/...' line)."""
    files = [l[6:].strip() for l in open(diff) if l.startswith("+++ b/")]
    if len(files) != 1 or os.path.dirname(files[0]) != CSRC.replace(os.sep, "/"):
        sys.exit("%s: a seeded fault is one diff against one file of %s" % (diff, CSRC))
    return os.path.basename(files[0])


def includes(path, seen):
    """Transitive closure of the #include "..." lines that stay inside csrc/."""
    for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(path).read(), re.M):
        p = os.path.normpath(os.path.join(os.path.dirname(path), inc))
        if os.path.dirname(p) == os.path.dirname(path) and p not in seen and os.path.exists(p):
            seen.add(p)
            includes(p, seen)
    return seen


def sources_that_include(name, srcs):
    base = os.path.join(ROOT, CSRC)
    hit = []
    for s in srcs:
        p = os.path.join(base, s)
        if s == name or os.path.join(base, name) in includes(p, set()):
            hit.append(s)
    return hit


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("names", nargs="*")
    ap.add_argument("-j", type=int, default=8, help="compiles in flight (at most 16)")
    a = ap.parse_args()
    jobs = max(1, min(a.j, 16))
    mk = makefile_vars()
    srcs = mk["SRCS"].split()
    names = a.names or sorted(os.path.basename(p)[:-5] for p in glob.glob(os.path.join(MUTANTS, "*.diff")))
    subprocess.check_call(["make", "-C", os.path.join(ROOT, CSRC), "-j%d" % jobs], stdout=subprocess.DEVNULL)
    os.makedirs(os.path.join(ROOT, "variants"), exist_ok=True)

    plan = {}      # name -> (scratch dir, recompiled sources)
    for n in names:
        diff = os.path.join(MUTANTS, n + ".diff")
        if not os.path.exists(diff):
            sys.exit("no such seeded fault: %s" % diff)
        tmp = os.path.join(ROOT, "variants", "src_" + n)
        shutil.rmtree(tmp, ignore_errors=True)
        os.makedirs(os.path.join(tmp, CSRC))
        shutil.copytree(os.path.join(ROOT, "include"), os.path.join(tmp, "include"))
        for f in os.listdir(os.path.join(ROOT, CSRC)):
            if f.endswith((".hip", ".h")):
                shutil.copy(os.path.join(ROOT, CSRC, f), os.path.join(tmp, CSRC, f))
        with open(diff) as fh:
            subprocess.check_call(["patch", "-p1", "-s", "--fuzz=0", "-d", tmp], stdin=fh)
        plan[n] = (tmp, sources_that_include(touched_file(diff), srcs))
        if not plan[n][1]:
            sys.exit("%s: no source of the Makefile includes the touched file" % n)

    def compile_one(task):
        n, s = task
        d = os.path.join(plan[n][0], CSRC)
        cmd = [mk["HIPCC"]] + mk["FLAGS"].split() + ["-c", s, "-o", s[:-4] + ".o"]
        r = subprocess.run(cmd, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        return n, s, r.returncode, r.stdout

    tasks = [(n, s) for n in names for s in plan[n][1]]
    failed = set()
    with concurrent.futures.ThreadPoolExecutor(jobs) as pool:
        for n, s, rc, out in pool.map(compile_one, tasks):
            if rc:
                failed.add(n)
                print("%s: %s does not compile\n%s" % (n, s, out), file=sys.stderr)
    for n in names:
        tmp, redo = plan[n]
        if n not in failed:
            objs = [os.path.join(tmp, CSRC, s[:-4] + ".o") if s in redo else os.path.join(ROOT, CSRC, s[:-4] + ".o") for s in srcs]
            lib = os.path.join(ROOT, "variants", "lib_%s.so" % n)
            subprocess.check_call([mk["HIPCC"], "--offload-arch=" + mk["ARCH"], "-shared", "-fPIC"] + objs + ["-o", lib])
            print("%-28s %-24s recompiled: %s" % (n, os.path.relpath(lib, ROOT), " ".join(redo)))
        shutil.rmtree(tmp)
    if failed:
        sys.exit("not built: %s" % " ".join(sorted(failed)))


if __name__ == "__main__":
    main()
