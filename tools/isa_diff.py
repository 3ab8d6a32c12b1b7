#!/usr/bin/env python3
"""Compare the device code of two builds kernel by kernel: the check that a refactor left the machine code alone.

    python tools/isa_diff.py DIR_A DIR_B

Each directory holds the device assembly of one revision's ``kernels/*.hip``, one ``.s`` per source file, made with
the release flags of ``csrc/build.py`` plus ``--offload-device-only -S``:

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -I csrc/include -D__HIP_PLATFORM_AMD__=1 \\
          --offload-device-only -S csrc/kernels/X.hip -o DIR/X.s

Per side the union over files of kernel symbol -> (instruction stream, resource metadata) is taken, so a kernel may
move between files.  Comments and assembler directives are dropped and local labels are renumbered in order of
appearance; the metadata is the VGPR / AGPR / SGPR counts, their spill counts, the LDS size and the scratch size of
the ``amdhsa.kernels`` notes.  Kernels in anonymous namespaces can share a mangled name across files: a name's
entries are compared as a multiset.  Exit status 0 iff both sides have the same symbols and every kernel is identical.
"""
from __future__ import annotations

import collections
import difflib
import glob
import os
import re
import sys

META = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count",
        ".group_segment_fixed_size", ".private_segment_fixed_size")
_LABEL = re.compile(r"\.L[A-Za-z_]+\d+(?:_\d+)?")


def _renumber(body):
    """Local labels (.LBB<function>_<block>, …) carry the function's index in its file: number them by first use."""
    names = {}
    return [_LABEL.sub(lambda m: names.setdefault(m.group(0), ".L%d" % len(names)), line) for line in body]


def parse(path):
    """-> {symbol: (tuple of instructions, tuple of metadata items)} for the kernels of one .s file."""
    bodies, meta = {}, {}
    name, body = None, []
    in_notes, cur = False, None
    with open(path, errors="replace") as f:
        for raw in f:
            line = raw.rstrip("\n")
            if in_notes:
                if line.startswith("  - "):
                    cur = {}
                    line = "    " + line[4:]
                if cur is not None and line.startswith("    .") and ":" in line:
                    k, v = line.strip().split(":", 1)
                    cur[k] = v.strip()
                    if k == ".name":
                        meta[cur[".name"]] = cur
                elif not line.startswith(" "):
                    in_notes, cur = False, None
                continue
            if line.startswith("amdhsa.kernels:"):
                in_notes = True
                continue
            if name is None:
                m = re.match(r"^([A-Za-z_][\w.$]*):", line)
                if m:
                    name, body = m.group(1), []
                continue
            if line.startswith(".Lfunc_end"):
                bodies[name] = body
                name = None
                continue
            code = line.split(";", 1)[0].strip()
            if not code:
                continue
            if code.endswith(":"):                      # a basic-block label
                body.append(code)
            elif not code.startswith("."):              # an instruction (directives start with a dot)
                body.append(re.sub(r"\s+", " ", code))
    out = {}
    for sym, m in meta.items():                         # kernels only: device functions have no notes entry
        if sym not in bodies:
            raise SystemExit(f"{path}: kernel {sym} has metadata but no body")
        out[sym] = (tuple(_renumber(bodies[sym])), tuple((k, m.get(k)) for k in META))
    return out


def side(d):
    files = sorted(glob.glob(os.path.join(d, "*.s")))
    if not files:
        raise SystemExit(f"no .s files in {d}")
    kernels = collections.defaultdict(list)
    for p in files:
        for sym, entry in parse(p).items():
            kernels[sym].append((entry, os.path.basename(p)))
    return kernels


def main(argv):
    if len(argv) != 3:
        print(__doc__)
        return 2
    a, b = side(argv[1]), side(argv[2])
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    for s in only_a:
        print(f"ONLY IN A  {s}  ({', '.join(f for _, f in a[s])})")
    for s in only_b:
        print(f"ONLY IN B  {s}  ({', '.join(f for _, f in b[s])})")
    total = same = 0
    for s in sorted(set(a) & set(b)):
        ea, eb = sorted(a[s]), sorted(b[s])
        total += max(len(ea), len(eb))
        if len(ea) != len(eb):
            print(f"COUNT      {s}: {len(ea)} in A, {len(eb)} in B")
        for (xa, fa), (xb, fb) in zip(ea, eb):
            if xa == xb:
                same += 1
                continue
            if xa[1] != xb[1]:
                print(f"METADATA   {s}  {fa}: {dict(xa[1])}  {fb}: {dict(xb[1])}")
            if xa[0] != xb[0]:
                d = list(difflib.unified_diff(xa[0], xb[0], fa, fb, lineterm="", n=1))
                print(f"CODE       {s}  ({len(xa[0])} / {len(xb[0])} instructions)")
                print("\n".join("    " + l for l in d[:40]))
    total += len(only_a) + len(only_b)
    print(f"{total} kernels, {same} identical")
    return 0 if same == total and not only_a and not only_b else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv))
