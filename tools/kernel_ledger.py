#!/usr/bin/env python3
"""Dispatches per kernel of the library's code objects in kernel-trace CSVs.

  rocprofv3 --kernel-trace --output-format csv -d TRACE -- python -m pytest -m gpu tests ...   (kernel trace only)
  python tools/kernel_ledger.py TRACE [TRACE2 ...] [--names FILE] [--require FILE]

Every *kernel_trace.csv under the given directories (or the given files) is read; a child process of the traced program leaves
a file of its own, and all of them count.  The kernels of the code objects are the names in --names (one per line, mangled or
demangled; written ahead of a GPU visit with --write-names), or, without it, those hipcc emits for engine.hip and multi.hip
(tests/isa_lib.py).  Kernels of other libraries in the trace are counted in one line.  Prints `count  kernel` for every kernel
and exits non-zero unless the kernels with no dispatch are exactly tests/kernel_ledger.py's UNLAUNCHED; with --require FILE,
also unless every kernel named in FILE (one per line) shows a dispatch."""
import argparse
import csv
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import isa_lib  # noqa: E402
import kernel_ledger as kl  # noqa: E402


def code_object_kernels(names_file):
    if names_file:
        with open(names_file) as f:
            raw = [ln.strip() for ln in f if ln.strip()]
    else:
        raw = list(isa_lib.kernel_meta(isa_lib.engine_isa())) + list(isa_lib.kernel_meta(isa_lib.multi_isa()))
    mangled = [n for n in raw if n.startswith("_Z")]
    plain = dict(zip(mangled, isa_lib.demangled(mangled))) if mangled else {}
    return sorted({kl.short_name(plain.get(n, n)) for n in raw})


def trace_files(paths):
    out = []
    for p in paths:
        if os.path.isdir(p):
            for d, _, files in os.walk(p):
                out += [os.path.join(d, f) for f in files if f.endswith("kernel_trace.csv")]
        else:
            out.append(p)
    return sorted(out)


def count_dispatches(files):
    counts, mangled = {}, {}
    for path in files:
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = row.get("Kernel_Name") or row.get("Name") or ""
                counts[name] = counts.get(name, 0) + 1
    for n in [n for n in counts if n.startswith("_Z")]:
        mangled[n] = None
    if mangled:
        for n, d in zip(list(mangled), isa_lib.demangled(list(mangled))):
            mangled[n] = d
    short = {}
    for n, c in counts.items():
        s = kl.short_name(mangled.get(n) or n)
        short[s] = short.get(s, 0) + c
    return short


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("traces", nargs="*")
    ap.add_argument("--names")
    ap.add_argument("--write-names", help="write the code objects' kernel names to this file and exit")
    ap.add_argument("--require")
    a = ap.parse_args()
    kernels = code_object_kernels(a.names)
    if a.write_names:
        with open(a.write_names, "w") as f:
            f.write("\n".join(kernels) + "\n")
        return 0
    files = trace_files(a.traces)
    if not files:
        print("no kernel_trace.csv found under", a.traces)
        return 2
    seen = count_dispatches(files)
    zero = sorted(k for k in kernels if not seen.get(k))
    other = {k: c for k, c in seen.items() if k not in kernels}
    print(f"# {len(files)} trace file(s), {sum(seen.values())} dispatches; {len(kernels)} kernels in the code objects, "
          f"{len(kernels) - len(zero)} with dispatches, {len(zero)} without")
    for k in kernels:
        print(f"{seen.get(k, 0):10d}  {k}")
    print(f"{sum(other.values()):10d}  ({len(other)} kernels of other libraries)")
    rc = 0
    if zero != sorted(kl.UNLAUNCHED):
        print("FAIL: no dispatch:", zero, "-- UNLAUNCHED:", sorted(kl.UNLAUNCHED))
        rc = 1
    if a.require:
        with open(a.require) as f:
            need = [kl.short_name(ln) for ln in f if ln.strip()]
        missing = [k for k in need if not seen.get(k)]
        print(f"# required: {len(need)} kernels, {len(need) - len(missing)} with dispatches")
        if missing:
            print("FAIL: required and not dispatched:", missing)
            rc = 1
    print("OK: the kernels without a dispatch are exactly UNLAUNCHED" if rc == 0 else "FAILED")
    return rc


if __name__ == "__main__":
    sys.exit(main())
