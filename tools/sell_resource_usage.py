#!/usr/bin/env python3
"""Resource usage of every spmv_sell_kernel and spmv_sell_persist_kernel instantiation, from the compiler's remarks on a gfx950 cross-compile (no GPU needed).

  tools/sell_resource_usage.py [csrc directory ...]      # default: this tree's krylov.jl_amd/csrc

Prints one row per instantiation: VGPRs, AGPRs, SGPRs, scratch bytes per lane, occupancy (waves per SIMD), LDS bytes.  With two
directories (another checkout's csrc first) the second table marks every row that differs from the first, so a change to the kernel
shows at once whether the other arms kept their registers.
"""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-I/opt/rocm/include", "--cuda-device-only",
         "-Rpass-analysis=kernel-resource-usage", "-x", "hip", "-c"]
KEYS = (("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("SGPRs", "sgpr"), ("ScratchSize [bytes/lane]", "scratch"), ("Occupancy [waves/SIMD]", "occ"),
        ("LDS Size [bytes/block]", "lds"))


def usage(csrc):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    err = subprocess.run([hipcc] + FLAGS + [os.path.join(csrc, "spmv.hip"), "-o", os.devnull], stderr=subprocess.PIPE, text=True, check=True).stderr
    out, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"remark: .*Function Name: (\S+)", line)
        if m:
            name = subprocess.run(["c++filt", m.group(1)], stdout=subprocess.PIPE, text=True).stdout.strip()
            cur = out.setdefault(name, {}) if re.search(r"spmv_sell(_persist)?_kernel<", name) else None
            continue
        if cur is None:
            continue
        for label, key in KEYS:
            m = re.search(r"remark: .*\s(?:Total)?" + re.escape(label) + r": (\d+)", line)
            if m:
                cur[key] = int(m.group(1))
    return out


def short(name):
    m = re.search(r"spmv_sell(_persist)?_kernel<([^>]*)>", name)
    return ("persist" if m.group(1) else "") + "<" + ", ".join("1" if v.strip() == "true" else "0" for v in m.group(2).split(",")) + ">"


def main():
    dirs = sys.argv[1:] or [os.path.join(ROOT, "krylov.jl_amd", "csrc")]
    prev = None
    for d in dirs:
        u = usage(d)
        print(f"# {os.path.relpath(d, ROOT) if len(dirs) == 1 else 'tree ' + str(dirs.index(d) + 1)}: {len(u)} instantiations of "
              "spmv_sell_kernel<DOT, COMP, DIST, NTM, COLS32, C4, PAIR, PAIRG[, ENT]> and spmv_sell_persist_kernel (persist<DOT, COMP, DIST, NTM, ONE>)")
        print(f"{'instantiation':<30}" + "".join(f"{k:>9}" for _, k in KEYS) + ("  vs tree 1" if prev is not None else ""))
        for name in sorted(u, key=short):
            row = u[name]
            mark = ""
            if prev is not None:
                key9 = short(name)
                old = next((r for n, r in prev.items() if short(n) == key9 or short(n)[:-1] + ", 0>" == key9), None)
                mark = "  new" if old is None else ("  same" if old == row else "  CHANGED " + str(old))
            print(f"{short(name):<30}" + "".join(f"{row.get(k, -1):>9}" for _, k in KEYS) + mark)
        prev = u
        print()


if __name__ == "__main__":
    main()
