"""Which kernel instantiations does the library hold, and which of them did a traced run launch?

  python tools/kernel_coverage.py compiled [SOURCE.hip ...]
      the kernel instantiations of gspn_amd/csrc/*.hip (or of the named sources), demangled, argument list stripped, one per line, sorted.
      Device code only (hipcc --cuda-device-only), so it runs without a GPU; the objects are kept under gspn_amd/csrc/build/cov/.
  python tools/kernel_coverage.py executed DIR... [--sources SOURCE.hip ...] [--expect FILE]
      DIR...: output directories of `rocprofv3 --kernel-trace --output-format csv -d DIR -- python -m pytest ...` (kernel tracing as the only
      tracing of the run; every CSV below them with a Kernel_Name column is read, child processes' included).  Prints per kernel template
      the number of instantiations compiled and executed, and the ones no trace holds.  --expect FILE (profiles/kernel_coverage_mlp.txt):
      exit status 1 if an instantiation of FILE's "[executed after]" section is in none of the traces.

Names only: nothing here looks inside a kernel."""
import argparse
import csv
import glob
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gspn_amd import build as B  # noqa: E402

COV = os.path.join(B.OBJ, "cov")
TARGET = "hip-amdgcn-amd-amdhsa--" + B.ARCH


def _tool(name):
    for d in (os.path.join(os.path.dirname(os.path.realpath(B.hipcc_path())), "..", "lib", "llvm", "bin"), "/opt/rocm/lib/llvm/bin", "/opt/rocm/llvm/bin"):
        p = os.path.join(d, name)
        if os.path.exists(p):
            return p
    return name


def _run(cmd, **kw):
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, **kw)
    if r.returncode != 0:
        raise RuntimeError("%s failed:\n%s" % (" ".join(cmd), r.stderr))
    return r.stdout


def demangle(names):
    names = list(names)
    todo = [n for n in names if n.startswith("_Z")]
    if not todo:
        return names
    out = _run(["c++filt"], input="\n".join(todo) + "\n").splitlines()
    table = dict(zip(todo, out))
    return [table.get(n, n) for n in names]


def strip_args(name):
    """'void ns::k<1, (anonymous namespace)::T>(int, float*) [clone .kd]' -> 'ns::k<1, (anonymous namespace)::T>'"""
    name = re.sub(r"\s*\[clone [^\]]*\]\s*$", "", name.strip())
    name = re.sub(r"\.kd$", "", name)
    depth, i, n = 0, 0, len(name)
    start = 0
    while i < n:
        c = name[i]
        if c == "<":
            depth += 1
        elif c == ">":
            depth -= 1
        elif c == " " and depth == 0:
            start = i + 1                                     # what came before was the return type
        elif c == "(" and depth == 0:
            if name.startswith("(anonymous namespace)", i):
                i += len("(anonymous namespace)")
                continue
            return re.sub(r"\s+", " ", name[start:i]).strip()
        i += 1
    return re.sub(r"\s+", " ", name[start:]).strip()


def normalise(names):
    return sorted({strip_args(n) for n in demangle(n.strip().strip('"') for n in names) if n.strip()})


def template_of(inst):
    """'ns::k<1, false>' -> 'ns::k'; '(anonymous namespace)::k<4>' -> '(anonymous namespace)::k' (the first '<' outside parentheses)"""
    depth = 0
    for i, c in enumerate(inst):
        if c == "(":
            depth += 1
        elif c == ")":
            depth -= 1
        elif c == "<" and depth == 0:
            return inst[:i]
    return inst


def device_symbols(src):
    """the *.kd symbols of one translation unit's gfx950 code object"""
    os.makedirs(COV, exist_ok=True)
    base = os.path.basename(src)[:-4]
    bundle, obj = os.path.join(COV, base + ".dev.o"), os.path.join(COV, base + "." + B.ARCH + ".o")
    hdrs = glob.glob(os.path.join(B.CSRC, "*.h")) + glob.glob(os.path.join(ROOT, "include", "*.h"))
    if B.newer(obj, [src] + hdrs):
        flags = list(B.FLAGS) + os.environ.get("GSPN_EXTRA_HIPCC_FLAGS", "").split()
        _run([B.hipcc_path()] + flags + ["--cuda-device-only", "-c", src, "-o", bundle])
        _run([_tool("clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + bundle, "--output=" + obj])
    syms = []
    for line in _run([_tool("llvm-readelf"), "-sW", obj]).splitlines():
        f = line.split()
        if len(f) >= 8 and f[-1].endswith(".kd"):
            syms.append(f[-1][:-3])
    return syms


def compiled(sources=()):
    srcs = sorted(glob.glob(os.path.join(B.CSRC, "*.hip")))
    if sources:
        want = {os.path.basename(s) for s in sources}
        missing = want - {os.path.basename(s) for s in srcs}
        if missing:
            raise SystemExit("no such source: %s" % ", ".join(sorted(missing)))
        srcs = [s for s in srcs if os.path.basename(s) in want]
    with ThreadPoolExecutor(max_workers=8) as ex:
        syms = [s for ss in ex.map(device_symbols, srcs) for s in ss]
    return normalise(syms)


def traced(dirs):
    csv.field_size_limit(1 << 30)
    names = set()
    nfiles = 0
    for top in dirs:
        paths = [top] if os.path.isfile(top) else [os.path.join(d, f) for d, _, fs in os.walk(top) for f in fs if f.endswith(".csv")]
        for p in sorted(paths):
            with open(p, newline="") as fh:
                rd = csv.DictReader(fh)
                if not rd.fieldnames or "Kernel_Name" not in rd.fieldnames:
                    continue
                nfiles += 1
                for row in rd:
                    if row["Kernel_Name"]:
                        names.add(row["Kernel_Name"])
    if not nfiles:
        raise SystemExit("no kernel-trace CSV (a Kernel_Name column) under %s" % " ".join(dirs))
    return normalise(names)


def read_section(path, title):
    """the names of section [title] of a coverage record: one per line, '#' starts a comment, the next '[' line ends it"""
    out, on = [], False
    with open(path) as fh:
        for line in fh:
            line = line.split("#", 1)[0].strip()
            if line.startswith("["):
                on = line.strip("[]").strip() == title
            elif on and line:
                out.append(line)
    return out


def report(comp, execd, out=sys.stdout):
    comp_set, ex_set = set(comp), set(execd)
    by = {}
    for c in comp:
        by.setdefault(template_of(c), []).append(c)
    out.write("%-34s %9s %9s\n" % ("kernel", "compiled", "executed"))
    for t in sorted(by):
        out.write("%-34s %9d %9d\n" % (t, len(by[t]), sum(1 for c in by[t] if c in ex_set)))
    out.write("%-34s %9d %9d\n" % ("total", len(comp), len(comp_set & ex_set)))
    miss = [c for c in comp if c not in ex_set]
    out.write("\nnot executed (%d):\n" % len(miss))
    for c in miss:
        out.write("  %s\n" % c)
    return miss


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    c = sub.add_parser("compiled")
    c.add_argument("sources", nargs="*", help="translation units by file name (default: all of gspn_amd/csrc)")
    e = sub.add_parser("executed")
    e.add_argument("dirs", nargs="+")
    e.add_argument("--sources", nargs="*", default=[], help="count against these translation units only")
    e.add_argument("--expect", help="coverage record whose [executed after] section must be in the traces")
    e.add_argument("--list", action="store_true", help="print the executed instantiations of the chosen sources, one per line, and nothing else")
    a = ap.parse_args(argv)
    if a.cmd == "compiled":
        print("\n".join(compiled(a.sources)))
        return 0
    comp = compiled(a.sources)
    execd = traced(a.dirs)
    if a.list:
        print("\n".join(x for x in execd if x in set(comp)))
        return 0
    report(comp, execd)
    if a.expect:
        gone = [n for n in read_section(a.expect, "executed after") if n not in set(execd)]
        if gone:
            print("\nexpected by %s, in no trace (%d):" % (a.expect, len(gone)))
            for n in gone:
                print("  " + n)
            return 1
        print("\nevery instantiation %s lists as executed is in the traces" % a.expect)
    return 0


if __name__ == "__main__":
    sys.exit(main())
