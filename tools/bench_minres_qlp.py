#!/usr/bin/env python3
"""minres_qlp! on the 512^3 Poisson operator and on the 256^3 one with an indefinite shift (λ = -0.5, inside the spectrum): ms per
iteration of the device-resident loop (path 2) and of the primitive sequence (path 0), alternated over --rounds pairs of --steps
iterations after a warm-up (atol = rtol = Artol = 0 and itmax = steps: every run does the full count), and, in the same process, the
same measurement of minres!'s and symmlq!'s path 2 (all three do one product per iteration; beside it minres_qlp! moves 104 n bytes
in its two passes and 8 n in the product's Lanczos epilogue, minres! 80 n + 8 n, symmlq! 80 n; minres_qlp!'s primitive sequence
232 n).
Prints one JSON line per operator; --out also writes them to a file (profiles/minres_qlp_bench.json).

    python tools/bench_minres_qlp.py --out profiles/minres_qlp_bench.json
    rocprofv3 --kernel-trace --stats ... -- python tools/bench_minres_qlp.py --operators poisson:512 --rounds 1 --no-path0 --no-minres     (per-kernel times; symmlq! stays in: its passes are the yardstick)
"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import krylov_jl_amd as K

ap = argparse.ArgumentParser()
ap.add_argument("--operators", nargs="+", default=["poisson:512", "poisson:256:-0.5"], help="kind:n1[:λ] of CsrMatrix.stencil")
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--no-path0", action="store_true")
ap.add_argument("--no-minres", action="store_true")
ap.add_argument("--no-symmlq", action="store_true")
ap.add_argument("--out", default=None)
a = ap.parse_args()

PASSES = 104                                           # P1 48 n + P2 56 n
ctx = K.Context(0)
lines = []
for spec in a.operators:
    kind, n1, *rest = spec.split(":")
    n1 = int(n1)
    lam = float(rest[0]) if rest else 0.0
    n = n1 ** 3
    A = K.CsrMatrix.stencil(ctx, kind, n1)
    x1 = ctx.empty(n); K.kfill_(x1, 1.0)
    b = A.matvec(x1)                                   # b = A ones
    del x1
    ws = K.MinresQlpWorkspace(ctx, n, n)

    def run(fused, steps):
        ctx.sync(); t0 = time.perf_counter()
        K.minres_qlp_(ws, A, b, fused=fused, itmax=steps, atol=0.0, rtol=0.0, Artol=0.0, λ=lam)
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
    fused_product = bool(ws.fused_product) if 2 in paths else None
    ctx.set_option("profile_spmv", 1)
    ctx.profile_kernels()
    wall, _ = run(2, a.steps)
    prof = ctx.profile_kernels()
    ctx.set_option("profile_spmv", 0)
    spmv_ms = prof["spmv"][1] / a.steps
    sb = A.spmv_bytes                                  # one product with A per iteration
    lz = 8 if ws.fused_product else 32                 # M⁻¹vₖ₋₁ inside the product, or the Lanczos pass of its own
    out = {"operator": kind, "n1": n1, "lambda": lam, "steps": a.steps, "rounds": a.rounds,
           "paths": {f"path{f}": v for f, v in paths.items()}, "fused_product": bool(ws.fused_product),
           "ms_per_iter": {f"path{f}": round(min(v), 4) for f, v in times.items()},
           "ms_per_iter_all": {f"path{f}": [round(t, 4) for t in v] for f, v in times.items()},
           "event_split_path2": {"spmv_ms_per_iter": round(spmv_ms, 4), "rest_ms_per_iter": round(wall - spmv_ms, 4)},
           "algorithmic_GB_per_iter": {"path2": round(((PASSES + lz) * n + sb) / 1e9, 3), "path0": round((232 * n + sb) / 1e9, 3)},
           "passes_GBps_from_event_split": round(PASSES * n / ((wall - spmv_ms) * 1e-3) / 1e9, 1),
           "spmv_bytes_one_product": sb}
    if 0 in times:
        pairs = [round(t2 / t0, 4) for t2, t0 in zip(times[2], times[0])]
        out["ratio_path2_over_path0_per_pair"] = pairs
        out["ratio_path2_over_path0"] = round(min(times[2]) / min(times[0]), 4)
        out["predicted_ratio_from_bytes"] = round(((PASSES + lz) * n + sb) / (232 * n + sb), 4)
        out["path2_faster_in_every_pair"] = all(p < 1.0 for p in pairs)
    del ws
    if not a.no_minres:                                # minres!'s device-resident loop on the same operator, same session
        wm = K.MinresWorkspace(ctx, n, n)

        def run_minres(steps):
            ctx.sync(); t0 = time.perf_counter()
            K.minres_(wm, A, b, fused=2, itmax=steps, atol=0.0, rtol=0.0, etol=0.0, conlim=0.0, λ=lam)
            ctx.sync()
            assert wm.stats.niter == steps and wm.last_path == 2, (wm.stats.niter, wm.stats.status, wm.last_path)
            return 1e3 * (time.perf_counter() - t0) / steps

        run_minres(a.warmup)
        tm = [run_minres(a.steps) for _ in range(a.rounds)]
        out["minres_path2_ms_per_iter"] = round(min(tm), 4)
        out["minres_path2_ms_per_iter_all"] = [round(t, 4) for t in tm]
        out["minres_fused_product"] = bool(wm.fused_product)
        out["minres_qlp_over_minres_path2"] = round(min(times[2]) / min(tm), 4)
        out["predicted_over_minres_from_bytes"] = round(((PASSES + lz) * n + sb) / ((80 + (8 if wm.fused_product else 32)) * n + sb), 4)
        del wm
    if not a.no_symmlq:                                # symmlq!'s device-resident loop likewise
        wq = K.SymmlqWorkspace(ctx, n, n)

        def run_symmlq(steps):
            ctx.sync(); t0 = time.perf_counter()
            K.symmlq_(wq, A, b, fused=2, itmax=steps, atol=0.0, rtol=0.0, etol=0.0, conlim=0.0, λ=lam)
            ctx.sync()
            assert wq.stats.niter == steps and wq.last_path == 2, (wq.stats.niter, wq.stats.status, wq.last_path)
            return 1e3 * (time.perf_counter() - t0) / steps

        run_symmlq(a.warmup)
        tq = [run_symmlq(a.steps) for _ in range(a.rounds)]
        out["symmlq_path2_ms_per_iter"] = round(min(tq), 4)
        out["symmlq_path2_ms_per_iter_all"] = [round(t, 4) for t in tq]
        out["minres_qlp_over_symmlq_path2"] = round(min(times[2]) / min(tq), 4)
        del wq
    lines.append(json.dumps(out))
    print(lines[-1], flush=True)
    del A, b
ctx.close()
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
