#!/usr/bin/env python3
"""CPU only: does a kernel-header edit change the machine code of the compiled-in kernels?  Compiles (nx, nu, N) translation units
for gfx950 from the working tree and from a git revision -- each exactly as csrc/gen_units.py writes it from that tree's
kernel_dims.txt / tile_dims.txt, tile-kernel forms included -- and compares every kernel's instruction stream and its
.amdhsa_* directives (registers, LDS, scratch); labels, comments and the other directives are ignored.  An edit that is meant to
touch only some variants can be proven not to touch the headline kernel without a GPU -- the measured numbers of an unchanged
instruction stream stay valid -- and a refactor can be proven to touch nothing at all.
    python tools/isa_diff.py [rev = HEAD] [nx nu N = 12 4 10]     one unit, one line per kernel
    python tools/isa_diff.py [rev = HEAD] --all                   every unit of either tree, one line per unit
    python tools/isa_diff.py [rev = HEAD] --names FILE            the run-time instantiated forms FILE names, one line per name
FILE holds one C++ instantiation name per line ('#' starts a comment: the format of csrc/jit_prebuilt.txt).  The library compiles
those forms on first use or at build time into the prebuilt store, never into a unit, so --all does not see them; each is compiled
here as an explicit instantiation, with the fused step blocks of its (nx, nu) defined as csrc/jit.hip defines them.
Exit status 1 when any kernel differs."""
import collections
import concurrent.futures
import difflib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tinympc_amd", "csrc")
sys.path.insert(0, CSRC)
import gen_units  # noqa: E402

SOURCES = ("admm_kernel.hip.h", "kernel_entry.hpp", "tile_kernel.hip.h", "kernel_dims.txt", "tile_dims.txt")
MAX_JOBS = 16          # compiles in flight (a fixed cap: the CPU count of a shared machine says nothing about this process's share)


def assemble(srcdir, name, text):
    """Compiles `text` as srcdir/_gen/<name>.hip with the Makefile's device flags; returns the assembly."""
    gen = os.path.join(srcdir, "_gen")
    os.makedirs(gen, exist_ok=True)
    with open(os.path.join(gen, name + ".hip"), "w") as f:
        f.write(text)
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", name + ".hip", "-o", name + ".s"],
                          cwd=gen, stderr=subprocess.DEVNULL)
    return open(os.path.join(gen, name + ".s")).read()


def read_names(path):
    """The instantiation names of a file in the format of csrc/jit_prebuilt.txt."""
    lines = (l.split("#")[0].strip() for l in open(path))
    return [l for l in lines if l]


def name_unit_text(name):
    """A unit that holds `name` alone, as an explicit instantiation (the headers are included as ../<name>, as in the generated units)."""
    m = re.match(r"(?:tinympc_amd::)?(admm_(?:tile|solve)_kernel)\s*<\s*(\d+)\s*,\s*(\d+)\s*,.*>$", name)
    if not m:
        raise SystemExit("isa_diff: not an instantiation of admm_tile_kernel / admm_solve_kernel: %r" % name)
    nx, nu = int(m.group(2)), int(m.group(3))
    fused = "#define TINYMPC_FUSED_NX %d\n#define TINYMPC_FUSED_NU %d\n" % (nx, nu) if nx + nu <= 16 else ""
    header = "tile_kernel.hip.h" if m.group(1) == "admm_tile_kernel" else "admm_kernel.hip.h"
    return '%s#include "../%s"\ntemplate __global__ void tinympc_amd::%s(const tinympc_amd::SolveArgs);\n' % (fused, header, name[name.index("admm_"):])


def kernels(text):
    """{kernel symbol: its instructions, then its .amdhsa_* lines} of one assembly file."""
    out = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)^\s*\.end_amdhsa_kernel", text, re.M | re.S):
        sym, desc = m.group(1), [l.strip() for l in m.group(2).splitlines() if l.strip()]
        start = re.search(r"^%s:[^\n]*\n" % re.escape(sym), text, re.M)
        end = text.find(".Lfunc_end", start.end())
        lines = [l.split(";")[0].strip() for l in text[start.end():end].splitlines()]
        out[sym] = [l for l in lines if l and not l.startswith(".") and not l.endswith(":")] + desc
    return out


def label(sym):
    a = [int(v) for v in re.findall(r"L[ib](\d+)E", sym)]
    return "<%d,%d,%d soc%d dbg%d mode%d lin%d het%d kmax%d>" % tuple(a[:9]) if "admm_solve_kernel" in sym and len(a) >= 9 else sym


def compare(a, b):
    """[(verdict, symbol, detail)] over the kernels of two assembly files; verdict: identical | CHANGED | added | removed."""
    res = []
    for sym in sorted(set(a) | set(b)):
        x, y = a.get(sym), b.get(sym)
        if x == y:
            res.append(("identical", sym, "%d instructions" % sum(1 for l in x if not l.startswith("."))))
        elif x is None or y is None:
            res.append(("added" if x is None else "removed", sym, ""))
        else:
            delta = collections.Counter(l.split()[0] for l in y)
            delta.subtract(collections.Counter(l.split()[0] for l in x))
            top = ", ".join(f"{k} {v:+d}" for k, v in sorted(delta.items(), key=lambda kv: -abs(kv[1]))[:6] if v)
            n = sum(1 for l in difflib.unified_diff(x, y, lineterm="", n=0) if l[:1] in "+-" and l[:3] not in ("+++", "---"))
            res.append(("CHANGED", sym, f"{len(x)} -> {len(y)} lines, {n} differing ({top})"))
    return res


def main():
    args = sys.argv[1:]
    every = "--all" in args
    names = None
    if "--names" in args:
        at = args.index("--names")
        if at + 1 >= len(args):
            raise SystemExit("isa_diff: --names needs a file")
        names = read_names(args[at + 1])
        del args[at:at + 2]
    args = [a for a in args if a != "--all"]
    rev = args[0] if args else "HEAD"
    with tempfile.TemporaryDirectory() as tmp:
        trees = {"old": os.path.join(tmp, "old"), "new": os.path.join(tmp, "new")}
        for side, d in trees.items():
            os.makedirs(d)
            for h in SOURCES:
                with open(os.path.join(d, h), "w") as f:
                    f.write(subprocess.check_output(["git", "show", "%s:tinympc_amd/csrc/%s" % (rev, h)], cwd=ROOT, text=True) if side == "old"
                            else open(os.path.join(CSRC, h)).read())
        dims = {side: gen_units.read_dims(d) for side, d in trees.items()}
        if names is not None:
            shapes = list(range(len(names)))              # (one unit per name, the same text for both trees)
        elif every:
            shapes = gen_units.unit_shapes(*dims["old"])
            shapes += [s for s in gen_units.unit_shapes(*dims["new"]) if s not in shapes]
        else:
            shapes = [tuple(int(v) for v in args[1:4]) if len(args) >= 4 else (12, 4, 10)]

        def one(job):
            side, shape = job
            if names is not None:
                return assemble(trees[side], "n_%d" % shape, name_unit_text(names[shape]))
            if shape not in gen_units.unit_shapes(*dims[side]):
                return ""
            return assemble(trees[side], "u_%d_%d_%d" % shape, gen_units.unit_text(shape, *dims[side]))
        jobs = [(side, shape) for shape in shapes for side in ("old", "new")]
        with concurrent.futures.ThreadPoolExecutor(min(MAX_JOBS, len(jobs))) as ex:
            asm = dict(zip(jobs, ex.map(one, jobs)))
    changed = total = 0
    for shape in shapes:
        res = compare(kernels(asm[("old", shape)]), kernels(asm[("new", shape)]))
        bad = [r for r in res if r[0] != "identical"]
        changed += len(bad)
        total += len(res)
        if names is not None:
            if not res:
                raise SystemExit("isa_diff: %r compiled to no kernel" % names[shape])
            res = [(v, names[shape], d) for v, sym, d in res]
        elif every:
            same_text = ", assembly byte-identical" if asm[("old", shape)] == asm[("new", shape)] else ""
            print("%-10s u_%d_%d_%d  %d kernels%s" % (("CHANGED" if bad else "identical",) + shape + (len(res), same_text if not bad else ", %d differ" % len(bad))))
        for verdict, sym, detail in (bad if every and names is None else res):
            print(f"{'    ' if every else ''}{verdict:<10} {label(sym)}  {detail}")
    what = "%d names" % len(names) if names is not None else ("%d units" % len(shapes) if every else shapes[0])
    print(f"{changed} of {total} variants of {what} differ from {rev}")
    return 1 if changed else 0


if __name__ == "__main__":
    sys.exit(main())
