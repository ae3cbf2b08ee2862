#!/usr/bin/env python3
"""cg_lanczos_shift! on the 512^3 Poisson operator for p shifts: ms per iteration of the device-resident loop (path 2) and of
the primitive sequence (path 0), alternated over rounds of --steps iterations after a warm-up (atol = rtol = 0: every run does
the full count); cg!'s ms per iteration times p (p separate solves); the HIP-event split of one profiled path-2 solve (SpMV
launches vs the rest); algorithmic bytes per iteration without the SpMV: path 2 (48 + 32p) n, path 0 (120 + 48p) n.  Prints one
JSON line per p."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import krylov_jl_amd as K

ap = argparse.ArgumentParser()
ap.add_argument("--n1", type=int, default=512)
ap.add_argument("--p", type=int, nargs="+", default=[1, 4, 8, 16])
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--no-path0", action="store_true")
a = ap.parse_args()

ctx = K.Context(0)
n = a.n1 ** 3
A = K.CsrMatrix.stencil(ctx, "poisson", a.n1)
x1 = ctx.empty(n); K.kfill_(x1, 1.0)
b = A.matvec(x1)                                   # b = A ones
del x1
ws_c = K.CgWorkspace(ctx, n, n)
kw = dict(atol=0.0, rtol=0.0)


def cg_ms(steps):
    ctx.sync(); t0 = time.perf_counter()
    K.cg_(ws_c, A, b, itmax=steps, **kw)
    ctx.sync()
    return 1e3 * (time.perf_counter() - t0) / ws_c.stats.niter


cg_ms(a.warmup)
cg = min(cg_ms(a.steps) for _ in range(a.rounds))
for p in a.p:
    shifts = list(np.logspace(-3, 1, p)) if p > 1 else [0.1]
    ws = K.CgLanczosShiftWorkspace(ctx, n, n, p)

    def run(fused, steps):
        ctx.sync(); t0 = time.perf_counter()
        K.cg_lanczos_shift_(ws, A, b, shifts, fused=fused, itmax=steps, **kw)
        ctx.sync()
        return 1e3 * (time.perf_counter() - t0) / ws.stats.niter, ws.last_path

    legs = (2,) if a.no_path0 else (2, 0)
    for f in legs:
        run(f, a.warmup)
    times, paths = {f: [] for f in legs}, {}
    for _ in range(a.rounds):
        for f in legs:
            t, paths[f] = run(f, a.steps)
            times[f].append(t)
    ctx.set_option("profile_spmv", 1)
    ctx.profile_kernels()
    wall, _ = run(2, a.steps)
    prof = ctx.profile_kernels()
    ctx.set_option("profile_spmv", 0)
    spmv_ms = prof["spmv"][1] / a.steps
    ms = {f"path{f}": round(min(v), 4) for f, v in times.items()}
    out = {"n1": a.n1, "p": p, "steps": a.steps, "rounds": a.rounds, "paths": {f"path{f}": v for f, v in paths.items()},
           "ms_per_iter": ms, "ms_per_iter_all": {f"path{f}": [round(t, 4) for t in v] for f, v in times.items()},
           "cg_ms_per_iter": round(cg, 4), "cg_ms_per_iter_times_p": round(cg * p, 4),
           "event_split_path2": {"spmv_ms_per_iter": round(spmv_ms, 4), "rest_ms_per_iter": round(wall - spmv_ms, 4)},
           "algorithmic_GB_per_iter_without_spmv": {"path2": round((48 + 32 * p) * n / 1e9, 3),
                                                   "path0": round((120 + 48 * p) * n / 1e9, 3)},
           "spmv_bytes": A.spmv_bytes}
    if 0 in times:
        out["speedup_path2_over_path0"] = round(min(times[0]) / min(times[2]), 4)
    print(json.dumps(out), flush=True)
    del ws
ctx.close()
