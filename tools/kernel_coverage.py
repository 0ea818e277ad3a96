#!/usr/bin/env python3
"""Which kernels of libal3d_hip.so has a run launched?

  kernel_coverage.py list [LIB]                 the library's kernel descriptors, one normalised name per line
  kernel_coverage.py diff [--lib LIB | --symbols FILE] [--by-file] TRACE...
                                                launched / never launched / launched but not in the library
  kernel_coverage.py trace OUTDIR -- CMD...     run one command under ``rocprofv3 --kernel-trace --stats`` (for the
                                                workers that tests start as child processes, should the profiler not
                                                follow them); prints the stats files it wrote

``list`` needs no GPU: it unbundles the gfx950 code objects (llvm-objdump --offloading), reads their ``.kd`` symbols
(llvm-readelf --dyn-syms) and demangles them.  A TRACE is a ``*_kernel_stats.csv`` of rocprofv3 (first column "Name"),
a directory searched for such files, or a plain text file with one kernel name per line.

Names are normalised the same way on both sides: return type and argument list stripped, template arguments kept (they
are part of the name), whitespace inside them made canonical."""
import argparse
import csv
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARCH = "gfx950"


def default_lib():
    hits = glob.glob(os.path.join(ROOT, "*", "csrc", "libal3d_hip.so"))
    return hits[0] if hits else os.path.join(ROOT, "libal3d_hip.so")


def _tool(name):
    for cand in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", name), name):
        path = shutil.which(cand)
        if path:
            return path
    raise SystemExit(f"kernel_coverage: {name} not found (looked in $ROCM_PATH/llvm/bin and on PATH)")


def normalize(name):
    """'void  k<64, 128 >(float const*, int) [clone .kd]' -> 'k<64,128>'."""
    s = name.strip().strip('"')
    s = re.sub(r"\s*\[clone [^\]]*\]$", "", s)
    if s.endswith(".kd"):
        s = s[:-3]
    s = re.sub(r"\s+", " ", s)
    m = re.match(r"_Z(\d+)", s)
    if m:                                                 # a name the demangler did not know (_Float16 arguments):
        a = m.end()                                       # a plain function's own name is spelled out in it
        base, rest = s[a:a + int(m.group(1))], s[a + int(m.group(1)):]
        if len(base) == int(m.group(1)) and not rest.startswith("I"):
            return base
    if s.endswith(")"):                                 # the argument list: the last top-level (...) group
        depth = 0
        for i in range(len(s) - 1, -1, -1):
            if s[i] == ")":
                depth += 1
            elif s[i] == "(":
                depth -= 1
                if depth == 0:
                    s = s[:i]
                    break
    # the return type of a template instantiation: everything before the last top-level space
    depth, cut = 0, -1
    for i, ch in enumerate(s):
        if ch in "<(":
            depth += 1
        elif ch in ">)":
            depth -= 1
        elif ch == " " and depth == 0:
            cut = i
    s = s[cut + 1:]
    s = re.sub(r"\s*([<>,])\s*", r"\1", s)
    return s.strip()


def demangle(names):
    tool = shutil.which(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-cxxfilt")) \
        or shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not tool:
        raise SystemExit("kernel_coverage: neither llvm-cxxfilt nor c++filt found")
    out = subprocess.run([tool], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout
    return out.splitlines()


def library_kernels(lib):
    """Sorted unique normalised names of the kernel descriptors in `lib`'s gfx950 code objects."""
    lib = os.path.abspath(lib)
    if not os.path.exists(lib):
        raise SystemExit(f"kernel_coverage: {lib} does not exist (build the library first)")
    mangled = set()
    with tempfile.TemporaryDirectory() as tmp:
        local = os.path.join(tmp, "lib.so")
        shutil.copy(lib, local)
        subprocess.run([_tool("llvm-objdump"), "--offloading", local], cwd=tmp, check=True, capture_output=True)
        objs = [p for p in glob.glob(os.path.join(tmp, "*")) if ARCH in os.path.basename(p)]
        if not objs:
            raise SystemExit(f"kernel_coverage: no {ARCH} code object in {lib}")
        for obj in objs:
            out = subprocess.run([_tool("llvm-readelf"), "--dyn-syms", "-W", obj], check=True, capture_output=True,
                                 text=True).stdout
            for line in out.splitlines():
                f = line.split()
                if f and f[-1].endswith(".kd"):
                    mangled.add(f[-1][:-3])
    return sorted({normalize(n) for n in demangle(sorted(mangled))})


def read_symbols(path):
    with open(path) as f:
        return sorted({normalize(l) for l in f if l.strip() and not l.startswith("#")})


def read_trace(path):
    """(normalised names, data rows) of one trace file."""
    names, rows = set(), 0
    with open(path, newline="") as f:
        first = f.readline()
        f.seek(0)
        if first.lstrip().startswith('"Name"') or first.lstrip().startswith("Name,"):
            for rec in csv.DictReader(f):
                if rec.get("Name"):
                    names.add(normalize(rec["Name"]))
                    rows += 1
        else:
            for line in f:
                if line.strip() and not line.startswith("#"):
                    names.add(normalize(line))
                    rows += 1
    return names, rows


def trace_files(paths):
    out = []
    for p in paths:
        if os.path.isdir(p):
            out += sorted(glob.glob(os.path.join(p, "**", "*kernel_stats.csv"), recursive=True))
        else:
            out.append(p)
    return out


def diff(library, traces):
    """-> dict(launched, never, foreign, rows): sorted lists of normalised names and {trace file: data rows}."""
    seen, rows = set(), {}
    for t in trace_files(traces):
        n, r = read_trace(t)
        seen |= n
        rows[t] = r
    lib = set(library)
    return dict(launched=sorted(lib & seen), never=sorted(lib - seen), foreign=sorted(seen - lib), rows=rows)


def source_of(names):
    """Normalised kernel name -> the csrc file that defines it (by its base name before '<')."""
    files = glob.glob(os.path.join(ROOT, "*", "csrc", "*.hip")) + glob.glob(os.path.join(ROOT, "*", "csrc", "*.h"))
    text = {os.path.basename(p): open(p).read() for p in files}
    out = {}
    for n in names:
        base = n.split("<")[0].split("::")[-1]
        pat = re.compile(r"__global__[^;{]{0,160}?\bvoid\s+" + re.escape(base) + r"\s*\(")
        out[n] = next((f for f, t in sorted(text.items()) if pat.search(t)), "?")
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("list")
    p.add_argument("lib", nargs="?", default=None)
    p = sub.add_parser("diff")
    p.add_argument("--lib", default=None)
    p.add_argument("--symbols", default=None, help="a text file of kernel names instead of a library")
    p.add_argument("--by-file", action="store_true", help="group the never-launched kernels by source file")
    p.add_argument("traces", nargs="+")
    p = sub.add_parser("trace")
    p.add_argument("outdir")
    p.add_argument("command", nargs=argparse.REMAINDER)
    a = ap.parse_args(argv)
    if a.cmd == "list":
        for n in library_kernels(a.lib or default_lib()):
            print(n)
        return 0
    if a.cmd == "trace":
        cmd = a.command[1:] if a.command[:1] == ["--"] else a.command
        if not cmd:
            raise SystemExit("kernel_coverage trace: no command after --")
        rc = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.outdir, "--",
                             *cmd]).returncode
        for f in trace_files([a.outdir]):
            print(f)
        return rc
    library = read_symbols(a.symbols) if a.symbols else library_kernels(a.lib or default_lib())
    d = diff(library, a.traces)
    print(f"# library: {len(library)} kernels; launched {len(d['launched'])}, never launched {len(d['never'])}, "
          f"launched but not in the library {len(d['foreign'])}")
    for t, r in d["rows"].items():
        print(f"# trace {os.path.basename(t)}: {r} rows")
    print("[launched]")
    print("\n".join(d["launched"]))
    print("[never launched]")
    if a.by_file:
        src = source_of(d["never"])
        for f in sorted(set(src.values())):
            print(f"{f}:")
            print("\n".join("  " + n for n in d["never"] if src[n] == f))
    else:
        print("\n".join(d["never"]))
    print("[launched, not in the library]")
    print("\n".join(d["foreign"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
