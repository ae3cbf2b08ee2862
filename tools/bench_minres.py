#!/usr/bin/env python3
"""minres! (device-resident loop) against cg! on the 512^3 Poisson operator, in one process: ms per iteration, alternated
rounds of --steps iterations after a warm-up, rtol = 1e-8 (the solves do not reach it within --steps: both run the full
count); the HIP-event split of one profiled solve of each (SpMV launches vs the rest of the iteration); algorithmic bytes
per iteration from the shapes.  Prints one JSON line."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import krylov_jl_amd as K

ap = argparse.ArgumentParser()
ap.add_argument("--n1", type=int, default=512)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--rounds", type=int, default=3)
a = ap.parse_args()

ctx = K.Context(0)
n = a.n1 ** 3
A = K.CsrMatrix.stencil(ctx, "poisson", a.n1)
x1 = ctx.empty(n); K.kfill_(x1, 1.0)
b = A.matvec(x1)                                   # b = A ones
del x1
ws_m = K.MinresWorkspace(ctx, n, n)
ws_c = K.CgWorkspace(ctx, n, n)
kw = dict(atol=0.0, rtol=1e-8)


def run(method, steps):
    if method == "minres":
        K.minres_(ws_m, A, b, itmax=steps, **kw)
        return ws_m.stats.niter, ws_m.last_path
    K.cg_(ws_c, A, b, itmax=steps, **kw)
    return ws_c.stats.niter, ws_c.last_path


for m in ("minres", "cg"):
    run(m, a.warmup)
times = {"minres": [], "cg": []}
paths = {}
for _ in range(a.rounds):
    for m in ("minres", "cg"):
        ctx.sync(); t0 = time.perf_counter()
        it, paths[m] = run(m, a.steps)
        ctx.sync()
        times[m].append(1e3 * (time.perf_counter() - t0) / it)
split = {}
ctx.set_option("profile_spmv", 1)
for m in ("minres", "cg"):
    ctx.profile_kernels()
    ctx.sync(); t0 = time.perf_counter()
    it, _ = run(m, a.steps)
    ctx.sync(); wall = 1e3 * (time.perf_counter() - t0) / it
    prof = ctx.profile_kernels()
    spmv_ms = prof["spmv"][1] / it
    split[m] = {"spmv_ms_per_iter": round(spmv_ms, 4), "spmv_launches_per_iter": prof["spmv"][0] / it,
                "rest_ms_per_iter": round(wall - spmv_ms, 4)}
ctx.set_option("profile_spmv", 0)
spmv_b = A.spmv_bytes
fused = ws_m.fused_product                          # the Lanczos step rides on the sliced SpMV: + r1 (8n) instead of a 32n pass
gb = {"minres": (spmv_b + (88 if fused else 112) * n) / 1e9,   # SpMV (+ P1) + P2 48n + P3 32n
      "cg": (spmv_b + 64 * n) / 1e9}             # fused SpMV + p.Ap, r -= alpha Ap ; r.r 24n, x, p update 40n
ms = {m: min(v) for m, v in times.items()}
print(json.dumps({"n1": a.n1, "steps": a.steps, "rounds": a.rounds, "paths": paths, "minres_fused_product": fused,
                  "ms_per_iter": {m: round(v, 4) for m, v in ms.items()},
                  "ms_per_iter_all": {m: [round(t, 4) for t in v] for m, v in times.items()},
                  "ratio_minres_over_cg": round(ms["minres"] / ms["cg"], 4), "target_ratio": 1.20,
                  "algorithmic_GB_per_iter": {m: round(v, 3) for m, v in gb.items()},
                  "predicted_ratio_from_bytes": round(gb["minres"] / gb["cg"], 4),
                  "event_split": split}), flush=True)
ctx.close()
