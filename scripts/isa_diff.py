#!/usr/bin/env python3
"""Per-kernel comparison of the gfx950 device code of two builds.  No GPU involved.

Build both trees with
    make -C nesti-net_amd/csrc EXTRA_CXXFLAGS=-save-temps=obj
then
    python scripts/isa_diff.py OLD/nesti-net_amd/csrc NEW/nesti-net_amd/csrc

Every *-hip-amdgcn-amd-amdhsa-gfx950.s is split per kernel symbol; comments, .file / .ident lines and the function index in
local labels (.LBB<n>_<m>: it changes when the kernels of a file are emitted in another order) are dropped.  Kernels are matched
by symbol over the whole library, so a kernel that moved to another source file is compared with itself.  Printed per source
file of the second build: kernels, identical, differing, moved (defined in another file of the first build); per differing
kernel: whether the opcode sequence is equal, the index of the first differing instruction and of the last v_mfma*, instruction
counts and the code-object metadata on both sides.
Exit status: 0 = same kernel symbols (whether or not their code differs), 1 = the symbol sets differ or a symbol is defined in
two files of one build, 2 = usage.
"""
import re
import shutil
import subprocess
import sys
from pathlib import Path

SUFFIX = "-hip-amdgcn-amd-amdhsa-gfx950.s"
META = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count",
        ".private_segment_fixed_size", ".group_segment_fixed_size")
COUNTED = ("v_mfma", "ds_read", "s_barrier", "s_waitcnt")
LABEL = re.compile(r"\.LBB\d+_(\d+)")


class Kernel:
    def __init__(self):
        self.lines = []      # normalised text of the body: instructions, labels, directives
        self.insts = []      # the instructions among them
        self.meta = {}

    def ops(self):
        return [i.split()[0] for i in self.insts]

    def count(self, prefix):
        return sum(1 for o in self.ops() if o.startswith(prefix))

    def last_mfma(self):
        idx = [i for i, o in enumerate(self.ops()) if o.startswith("v_mfma")]
        return idx[-1] if idx else -1


def parse(path):
    """{kernel symbol: Kernel} of one assembly file."""
    text = path.read_text().splitlines()
    names = {l.split()[1] for l in text if l.lstrip().startswith(".amdhsa_kernel ")}
    kernels, cur = {}, None
    entry = None             # the metadata entry being read
    for raw in text:
        m = re.match(r"^  - (\.\w+):\s*(.*)$", raw) or re.match(r"^    (\.\w+):\s*(.*)$", raw)
        if m:
            if raw.startswith("  - "):
                entry = {}
            if entry is not None:
                entry[m.group(1)] = m.group(2).strip()
                if m.group(1) == ".name" and entry[".name"].strip("'\"") in kernels:
                    kernels[entry[".name"].strip("'\"")].meta = entry
            continue
        line = raw.split(";", 1)[0].strip()
        if not line or line.startswith((".file", ".ident")):
            continue
        if cur is None:
            if line.endswith(":") and line[:-1] in names:
                cur = kernels[line[:-1]] = Kernel()
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        line = LABEL.sub(r".LBB_\1", line)
        cur.lines.append(line)
        if not line.startswith(".") and not line.endswith(":"):
            cur.insts.append(line)
    return kernels


def load(root):
    """({kernel symbol: (source file, Kernel)}, [symbols defined in two files]) of every assembly file under root."""
    out, twice = {}, []
    for f in sorted(Path(root).rglob("*" + SUFFIX)):
        for sym, k in parse(f).items():
            if sym in out:
                twice.append(f"{sym}: {out[sym][0]}.hip and {f.name[:-len(SUFFIX)]}.hip")
            out[sym] = (f.name[:-len(SUFFIX)], k)
    return out, twice


def demangle(syms):
    tool = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not tool or not syms:
        return {s: s for s in syms}
    res = subprocess.run([tool], input="\n".join(syms), capture_output=True, text=True)
    names = res.stdout.splitlines()
    return dict(zip(syms, names)) if len(names) == len(syms) else {s: s for s in syms}


def pair(a, b):
    return f"{a}" if a == b else f"{a} -> {b}"


def main(argv):
    if len(argv) != 3:
        print(__doc__)
        return 2
    (old, old_twice), (new, new_twice) = load(argv[1]), load(argv[2])
    if not old or not new:
        print(f"no *{SUFFIX} under one of the directories: build with EXTRA_CXXFLAGS=-save-temps=obj")
        return 2
    status = 1 if old_twice or new_twice else 0
    details = [f"defined twice in the {n} build: {t}" for n, ts in (("first", old_twice), ("second", new_twice)) for t in ts]
    if set(old) != set(new):
        status = 1
        details += [f"{old[s][0]}.hip: only in the first build: {s}" for s in sorted(set(old) - set(new))]
        details += [f"{new[s][0]}.hip: only in the second build: {s}" for s in sorted(set(new) - set(old))]
    both = sorted(set(old) & set(new))
    total = [0, 0, 0, 0]
    print(f"{'file':<14}{'kernels':>8}{'identical':>11}{'differing':>11}{'moved':>7}")
    for src in sorted({new[s][0] for s in both}):
        here = [s for s in both if new[s][0] == src]
        ko, kn = {s: old[s][1] for s in here}, {s: new[s][1] for s in here}
        diff = [s for s in here
                if ko[s].lines != kn[s].lines or any(ko[s].meta.get(m) != kn[s].meta.get(m) for m in META)]
        moved = [s for s in here if old[s][0] != src]
        print(f"{src + '.hip':<14}{len(here):>8}{len(here) - len(diff):>11}{len(diff):>11}{len(moved):>7}")
        for i, n in enumerate((len(here), len(here) - len(diff), len(diff), len(moved))):
            total[i] += n
        for frm in sorted({old[s][0] for s in moved}):
            details.append(f"{src}.hip: {sum(1 for s in moved if old[s][0] == frm)} kernels moved here from {frm}.hip")
        pretty = demangle(diff)
        for s in diff:
            a, b = ko[s], kn[s]
            oa, ob = a.ops(), b.ops()
            first = next((i for i, (x, y) in enumerate(zip(a.insts, b.insts)) if x != y), min(len(a.insts), len(b.insts)))
            first_op = next((i for i, (x, y) in enumerate(zip(oa, ob)) if x != y), min(len(oa), len(ob)))
            details.append(f"{src}.hip  {pretty[s]}")
            details.append(f"    opcode sequence {'equal' if oa == ob else 'differs (first at ' + str(first_op) + ')'}; "
                           f"first differing instruction {first}; last v_mfma at {pair(a.last_mfma(), b.last_mfma())}; "
                           f"instructions {pair(len(oa), len(ob))}")
            details.append("    " + "  ".join(f"{c}* {pair(a.count(c), b.count(c))}" for c in COUNTED))
            details.append("    " + "  ".join(f"{m} {pair(a.meta.get(m), b.meta.get(m))}" for m in META))
    print(f"{'total':<14}{total[0]:>8}{total[1]:>11}{total[2]:>11}{total[3]:>7}")
    if details:
        print()
        print("\n".join(details))
    print()
    print("kernel symbol sets: " + ("equal" if status == 0 else "DIFFERENT"))
    return status


if __name__ == "__main__":
    sys.exit(main(sys.argv))
