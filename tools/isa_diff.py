#!/usr/bin/env python3
"""Did the kernels change?  Compares two assembly files of engine.hip (hipcc -S with the flags of tests/isa_lib.py, one
from the parent commit and one from the working tree) kernel by kernel: the instructions as text, modulo the function's
number in the code object (branch targets keep their block index and lose that number: isa_lib.kernel_bodies), and the
metadata (registers, spills, scratch, LDS) as they are.  Where a kernel stands in the code object is therefore no
difference; one line says whether the kernels both sides have are emitted in the same order (information only).

    python tools/isa_diff.py parent.s new.s --must-match k_blind_rotateILi2ELi10E --must-match k_keyswitch

Exit status 1 if a kernel whose mangled name contains a --must-match substring differs, or is on one side only."""
import argparse
import difflib
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from isa_lib import kernel_bodies, kernel_meta  # noqa: E402


def changed_lines(a, b):
    """lines of either side that are not part of the longest common subsequence, counted once per replaced pair"""
    ops = difflib.SequenceMatcher(None, a, b, autojunk=False).get_opcodes()
    return sum(max(i2 - i1, j2 - j1) for tag, i1, i2, j1, j2 in ops if tag != "equal")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--must-match", action="append", default=[], metavar="SUBSTRING")
    args = ap.parse_args()
    old, new = open(args.old).read(), open(args.new).read()
    bodies = kernel_bodies(old), kernel_bodies(new)
    meta = kernel_meta(old), kernel_meta(new)
    same = different = meta_changed = failed = 0
    for name in sorted(set(bodies[0]) | set(bodies[1])):
        must = any(s in name for s in args.must_match)
        if name not in bodies[0] or name not in bodies[1]:
            print(f"ONLY IN {'old' if name in bodies[0] else 'new'}  {name}")
            different += 1
            failed += must
            continue
        a, b = bodies[0][name], bodies[1][name]
        ma, mb = meta[0].get(name), meta[1].get(name)
        meta_changed += ma != mb
        if a == b and ma == mb:
            same += 1
            print(f"identical  {name}  ({len(a)} instructions)")
            continue
        different += 1
        failed += must
        print(f"DIFFERENT{' (must match)' if must else ''}  {name}: {len(a)} -> {len(b)} instructions, "
              f"{changed_lines(a, b)} changed lines")
        print(f"    old {ma}\n    new {mb}")
    order = [[k for k in b if k in bodies[0] and k in bodies[1]] for b in bodies]
    moved = next((i for i, (a, b) in enumerate(zip(*order)) if a != b), None)
    if moved is None:
        print(f"order: the {len(order[0])} common kernels are emitted in the same order")
    else:
        print(f"order: changed, first at index {moved} of {len(order[0])} common kernels: {order[0][moved]} -> {order[1][moved]}")
    print(f"summary: {same} identical, {different} different, {meta_changed} with changed metadata, "
          f"{failed} must-match failures")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
