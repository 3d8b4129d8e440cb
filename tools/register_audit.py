#!/usr/bin/env python3
"""CPU only: register / scratch / occupancy report of every kernel instantiation compiled into the library
(hipcc -Rpass-analysis=kernel-resource-usage on tinympc_amd/csrc/_gen/{k,t}_*.hip).  Scratch > 0 = spilled to memory.
The one-row forms csrc/jit_prebuilt.txt names (run-time instantiated, never in a unit) are compiled here as explicit instantiations and
listed after the compiled-in ones; then the setup kernels of batch_dispatch.hip (riccati_kernel, sensitivity_kernel) and, last, the helper
kernels of batch_instance.hip (the fill kernels of the per-instance data) and of batch_closed_loop.hip (the fill kernels of the closed-loop
stages and of the generated noise, the coverage path's helpers -- fill_actuator_kernel, write_actuator_launch_kernel and
coverage_actuator_kernel of the actuator model among them).
    python tools/register_audit.py [--all] > profiles/rNN_register_audit.md"""
import concurrent.futures
import glob
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tinympc_amd", "csrc")
GEN = os.path.join(CSRC, "_gen")


def usage(src, cwd=GEN, extra=()):
    with tempfile.TemporaryDirectory() as tmp:
        p = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage", *extra,
                            "-c", src, "-o", os.path.join(tmp, "o.o")], capture_output=True, text=True, cwd=cwd)
    rows = []
    for b in p.stderr.split("Function Name:")[1:]:
        name = b.split()[0]
        g = lambda k: int(re.search(k + r": (\d+)", b).group(1))
        rows.append(dict(kind="tile" if "tile_kernel" in name else "one-row", name=name, args=[int(v) for _, v in re.findall(r"L([ib])(\d+)E", name)],
                         vgpr=g("VGPRs"), agpr=g("AGPRs"), scratch=g(r"ScratchSize \[bytes/lane\]"), occ=g(r"Occupancy \[waves/SIMD\]"),
                         lds=g(r"LDS Size \[bytes/block\]")))
    return rows


def prebuilt_one_row_rows():
    """the one-row forms of csrc/jit_prebuilt.txt, each compiled as an explicit instantiation with its shape's fused step blocks"""
    names = [l.split("#")[0].strip() for l in open(os.path.join(CSRC, "jit_prebuilt.txt"))]
    rows = []
    for n in (n for n in names if "admm_solve_kernel<" in n):
        nx, nu = (int(v) for v in re.match(r".*admm_solve_kernel<\s*(\d+)\s*,\s*(\d+)", n).groups())
        with tempfile.NamedTemporaryFile("w", suffix=".hip", dir=GEN, delete=False) as f:
            f.write('#define TINYMPC_FUSED_NX %d\n#define TINYMPC_FUSED_NU %d\n#include "../admm_kernel.hip.h"\n'
                    'template __global__ void tinympc_amd::%s(const tinympc_amd::SolveArgs);\n' % (nx, nu, n[n.index("admm_"):]))
        try:
            rows += usage(f.name)
        finally:
            os.unlink(f.name)
    return rows


def setup_kernel_rows():
    """riccati_kernel / sensitivity_kernel: device code of batch_dispatch.hip"""
    return [r for r in usage("batch_dispatch.hip", cwd=CSRC, extra=("--cuda-device-only",)) if re.search(r"riccati_kernel|sensitivity_kernel", r["name"])]


def helper_kernel_rows():
    """every __global__ of batch_instance.hip (the per-instance fill kernels) and of batch_closed_loop.hip: fill kernels
    (generate_diagonal_kernel / generate_factor_kernel, fill_actuator_kernel among them) and coverage helpers (coverage_actuator_kernel:
    the actuator model behind a coverage launch)"""
    return [r for unit in ("batch_instance.hip", "batch_closed_loop.hip") for r in usage(unit, cwd=CSRC, extra=("--cuda-device-only",))]


def main():
    srcs = sorted(glob.glob(os.path.join(GEN, "u_*.hip")))
    if not srcs:
        sys.exit("build the library first (tinympc_amd/csrc/_gen is empty)")
    with concurrent.futures.ThreadPoolExecutor(8) as ex:
        rows = [r for rs in ex.map(usage, srcs) for r in rs]
    show_all = "--all" in sys.argv
    print(f"{len(rows)} kernel instantiations, {sum(r['scratch'] > 0 for r in rows)} with scratch (memory spills)\n")
    print("one-row kernel `admm_solve_kernel<NX,NU,N,SOC,DBG,MODE,LIN,HET,KMAX,ADAPT,UB,HALF,PF>` -- default variants (box constraints, MODE 2; UB = the form launched when the box is the same at every knot), cone and adaptive-rho variants:\n")
    print("| (nx,nu,N) | variant | VGPR | AGPR | scratch B/lane | waves/SIMD | LDS B |")
    print("|---|---|---|---|---|---|---|")
    for r in sorted((r for r in rows if r["kind"] == "one-row"), key=lambda r: (r["args"][:3], r["args"][3:])):
        a = r["args"]
        # <NX,NU,N, SOC,DBG,MODE,LIN,HET, KMAX, ADAPT, UB>
        extra = tuple(a[9:11]) if len(a) >= 11 else (0, 0)
        tag = {((0, 0, 2, 0, 0), (0, 0)): "box", ((0, 0, 2, 0, 0), (0, 1)): "box, knot-invariant (UB)", ((1, 0, 2, 0, 0), (0, 0)): "cone",
               ((0, 0, 2, 0, 0), (1, 0)): "adaptive rho"}.get((tuple(a[3:8]), extra))
        if tag is None and not show_all:
            continue
        tag = tag or f"soc{a[3]} dbg{a[4]} mode{a[5]} lin{a[6]} het{a[7]} adapt{extra[0]} ub{extra[1]}"
        # (round 4: HALF rows, round 6: the PREFETCH form -- template arguments 12 and 13)
        if len(a) >= 12 and a[11]:
            tag += ", HALF rows"
        if len(a) >= 13 and a[12]:
            tag += ", PREFETCH form"
        print(f"| ({a[0]},{a[1]},{a[2]}) | {tag} | {r['vgpr']} | {r['agpr']} | {r['scratch']} | {r['occ']} | {r['lds']} |")
    pre = prebuilt_one_row_rows()
    if pre:
        print("\none-row forms of csrc/jit_prebuilt.txt (run-time instantiated; HET = per-instance problem data, ADAPT = adaptive rho):\n")
        print("| (nx,nu,N) | variant | VGPR | AGPR | scratch B/lane | waves/SIMD | LDS B |")
        print("|---|---|---|---|---|---|---|")
        for r in pre:
            a = r["args"]
            print(f"| ({a[0]},{a[1]},{a[2]}) | soc{a[3]} dbg{a[4]} mode{a[5]} lin{a[6]} het{a[7]} adapt{a[9]} | {r['vgpr']} | {r['agpr']} | {r['scratch']} | {r['occ']} | {r['lds']} |")
    print("\ntile kernel `admm_tile_kernel<NX,NU,N,W,R>`:\n")
    print("| (nx,nu,N) | W x R | form | VGPR | AGPR | scratch B/lane | waves/SIMD | LDS B |")
    print("|---|---|---|---|---|---|---|---|")
    for r in sorted((r for r in rows if r["kind"] == "tile"), key=lambda r: r["args"]):
        a = r["args"]
        form = "box in registers (UB)" if len(a) >= 9 and a[8] else "box table in LDS"
        print(f"| ({a[0]},{a[1]},{a[2]}) | {a[3]} x {a[4]} | {form} | {r['vgpr']} | {r['agpr']} | {r['scratch']} | {r['occ']} | {r['lds']} |")
    print("\nsetup kernels of batch_dispatch.hip (one wavefront per instance; their LDS is dynamic, sized by the shape at launch):\n")
    print("| kernel | VGPR | AGPR | scratch B/lane | waves/SIMD | static LDS B |")
    print("|---|---|---|---|---|---|")
    for r in setup_kernel_rows():
        kname = "sensitivity_kernel" if "sensitivity_kernel" in r["name"] else "riccati_kernel"
        print(f"| {kname} | {r['vgpr']} | {r['agpr']} | {r['scratch']} | {r['occ']} | {r['lds']} |")
    print("\nhelper kernels of batch_instance.hip and batch_closed_loop.hip (256 threads a block, grid-stride):\n")
    print("| kernel | VGPR | AGPR | scratch B/lane | waves/SIMD | LDS B |")
    print("|---|---|---|---|---|---|")
    for r in helper_kernel_rows():
        kname = re.search(r"tinympc_amdL?\d+([a-z_]+_kernel)", r["name"])
        print(f"| {kname.group(1) if kname else r['name']} | {r['vgpr']} | {r['agpr']} | {r['scratch']} | {r['occ']} | {r['lds']} |")


if __name__ == "__main__":
    main()
