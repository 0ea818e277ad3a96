#!/usr/bin/env python3
"""Dev tool: compare two device-only assembly files (hipcc --cuda-device-only -S) symbol by symbol.

    python tools/asm_symbol_diff.py before.s after.s

A file is cut into blocks: the text of every function (from its `.globl` / `.type` lines to its `.Lfunc_end` label), the
`.amdhsa_kernel` descriptor of every kernel (registers, LDS, scratch), every data object, and the metadata note.  Blocks
are matched by name, so the position of a block in the file does not count; the `__hip_cuid_*` symbol (a hash of the
compilation unit) is left out.  Prints the names of the blocks that differ or exist on one side only and exits 1 if
there are any.  It is a diff, nothing more."""
import re
import sys

SKIP = re.compile(r"__hip_cuid_|^\s*\.ident|^\s*\.file")


def blocks(path):
    out, name, cur = {}, "<preamble>", []
    lines = [l.rstrip() for l in open(path) if not SKIP.search(l)]
    for i, l in enumerate(lines):
        m = (re.match(r"\s*\.(?:globl|weak|protected|hidden)\s+(\S+)", l) if not re.match(r"\s*\.(?:globl|weak|protected|hidden)", lines[i - 1] if i else "")
             else None)
        k = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)
        t = re.match(r"\s*\.type\s+(\S+),@(?:object|function)", l)
        a = re.match(r"\s*\.amdgpu_metadata", l)
        new = ("sym " + m.group(1)) if m else ("desc " + k.group(1)) if k else ("<metadata>" if a else None)
        if new is None and t and ("sym " + t.group(1)) != name:
            new = "sym " + t.group(1)
        if new is not None and new != name:
            out.setdefault(name, []).extend(cur)
            name, cur = new, []
        cur.append(l)
    out.setdefault(name, []).extend(cur)
    return out


def main():
    a, b = blocks(sys.argv[1]), blocks(sys.argv[2])
    bad = [n for n in sorted(set(a) | set(b)) if a.get(n) != b.get(n)]
    kernels = sum(1 for n in a if n.startswith("desc "))
    print(f"{sys.argv[1]}: {len(a)} blocks, {kernels} kernel descriptors; {len(bad)} blocks differ")
    for n in bad:
        print("  " + n + ("" if n in a and n in b else "  (one side only)"))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
