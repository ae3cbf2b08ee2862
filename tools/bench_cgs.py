#!/usr/bin/env python3
"""cgs! on the 512^3 Poisson operator and on kron_unsymmetric(256): ms per iteration of the device-resident loop (path 2) and of
the primitive sequence (path 0), alternated over --rounds pairs of --steps iterations after a warm-up (atol = rtol = 0 and
itmax = steps: every run does the full count), and, in the same process, the same measurement of bicgstab!'s path 2 (both do two
products per iteration; cgs! moves 120 n bytes beside them, its primitive sequence 240 n, bicgstab! 128 n).
Prints one JSON line per operator; --out also writes them to a file (profiles/cgs_bench.json).

    python tools/bench_cgs.py --out profiles/cgs_bench.json
    rocprofv3 --kernel-trace --stats ... -- python tools/bench_cgs.py --operators poisson:512 --rounds 1 --no-path0 --no-bicgstab     (per-kernel times)
"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import krylov_jl_amd as K

ap = argparse.ArgumentParser()
ap.add_argument("--operators", nargs="+", default=["poisson:512", "kron_unsymmetric:256"], help="kind:n1 of CsrMatrix.stencil")
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--no-path0", action="store_true")
ap.add_argument("--no-bicgstab", action="store_true")
ap.add_argument("--out", default=None)
a = ap.parse_args()

ctx = K.Context(0)
lines = []
for spec in a.operators:
    kind, n1 = spec.split(":")
    n1 = int(n1)
    n = n1 ** 3
    A = K.CsrMatrix.stencil(ctx, kind, n1)
    x1 = ctx.empty(n); K.kfill_(x1, 1.0)
    b = A.matvec(x1)                                   # b = A ones
    del x1
    ws = K.CgsWorkspace(ctx, n, n)

    def run(fused, steps):
        ctx.sync(); t0 = time.perf_counter()
        K.cgs_(ws, A, b, fused=fused, itmax=steps, atol=0.0, rtol=0.0)
        ctx.sync()
        st = ws.stats
        assert st.niter == steps, (st.niter, st.status)
        return 1e3 * (time.perf_counter() - t0) / st.niter, ws.last_path

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
    sb = 2 * A.spmv_bytes                              # two products with A per iteration
    out = {"operator": kind, "n1": n1, "steps": a.steps, "rounds": a.rounds, "paths": {f"path{f}": v for f, v in paths.items()},
           "ms_per_iter": {f"path{f}": round(min(v), 4) for f, v in times.items()},
           "ms_per_iter_all": {f"path{f}": [round(t, 4) for t in v] for f, v in times.items()},
           "event_split_path2": {"spmv_ms_per_iter": round(spmv_ms, 4), "rest_ms_per_iter": round(wall - spmv_ms, 4)},
           "algorithmic_GB_per_iter": {"path2": round((120 * n + sb) / 1e9, 3), "path0": round((240 * n + sb) / 1e9, 3)},
           "spmv_bytes_two_products": sb}
    if 0 in times:
        pairs = [round(t2 / t0, 4) for t2, t0 in zip(times[2], times[0])]
        out["ratio_path2_over_path0_per_pair"] = pairs
        out["ratio_path2_over_path0"] = round(min(times[2]) / min(times[0]), 4)
        out["predicted_ratio_from_bytes"] = round((120 * n + sb) / (240 * n + sb), 4)
        out["path2_faster_in_every_pair"] = all(p < 1.0 for p in pairs)
    del ws
    if not a.no_bicgstab:                              # bicgstab!'s device-resident loop on the same operator, same session
        wb = K.BicgstabWorkspace(ctx, n, n)

        def run_bicgstab(steps):
            ctx.sync(); t0 = time.perf_counter()
            K.bicgstab_(wb, A, b, fused=2, itmax=steps, atol=0.0, rtol=0.0)
            ctx.sync()
            assert wb.stats.niter == steps and wb.last_path == 2, (wb.stats.niter, wb.stats.status, wb.last_path)
            return 1e3 * (time.perf_counter() - t0) / steps

        run_bicgstab(a.warmup)
        tb = [run_bicgstab(a.steps) for _ in range(a.rounds)]
        out["bicgstab_path2_ms_per_iter"] = round(min(tb), 4)
        out["bicgstab_path2_ms_per_iter_all"] = [round(t, 4) for t in tb]
        out["cgs_over_bicgstab_path2"] = round(min(times[2]) / min(tb), 4)
        out["predicted_cgs_over_bicgstab_from_bytes"] = round((120 * n + sb) / (128 * n + sb), 4)
        del wb
    lines.append(json.dumps(out))
    print(lines[-1], flush=True)
    del A, b
ctx.close()
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
