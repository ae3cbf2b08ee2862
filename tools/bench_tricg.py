#!/usr/bin/env python3
"""tricg! on the 512^3 Poisson operator and on kron_unsymmetric(256) with c = A' b (A' built by transpose()): ms per iteration of the
device-resident loop (path 2) and of the primitive sequence (path 0), alternated over --rounds pairs of --steps iterations after a
warm-up (atol = rtol = 0 and itmax = steps: every run does the full count), and, in the same process, trilqr! on its path 2 as the
yardstick: the code of the parent commit on the same driver (tricg! moves 248 n bytes per iteration beside two products, its
primitive sequence 480 n; trilqr! 224 n).
One more path-2 solve of each runs with the HIP-event brackets on (khip_profile_kernels): the products and each of the three passes,
as ms per launch and as TB/s on the pass's bytes (P1 56 n, P2 48 n, P3 144 n; the lighter P1 and P3 of the first iteration are in
the mean), with trilqr!'s P3 (120 n) beside tricg!'s.
Prints one JSON line per operator; --out also writes them to a file (profiles/tricg_bench.json).

    python tools/bench_tricg.py --out profiles/tricg_bench.json
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
ap.add_argument("--no-siblings", action="store_true")
ap.add_argument("--out", default=None)
a = ap.parse_args()

PASS_BYTES = {"ssy_p1": 56, "ssy_p2": 48, "tricg_p3": 144}       # per entry of a vector
FUSED_BYTES, PRIMITIVE_BYTES, TRILQR_FUSED_BYTES = 248, 480, 224
ctx = K.Context(0)
lines = []
for spec in a.operators:
    kind, n1 = spec.split(":")
    n1 = int(n1)
    n = n1 ** 3
    A = K.CsrMatrix.stencil(ctx, kind, n1)
    At = A.transpose()
    x1 = ctx.empty(n); K.kfill_(x1, 1.0)
    b = A.matvec(x1)                                   # b = A ones
    del x1
    c = At.matvec(b)                                   # c = A' b
    ws = K.TricgWorkspace(ctx, n, n)

    def run(fused, steps):
        ctx.sync(); t0 = time.perf_counter()
        K.tricg_(ws, A, b, c, At=At, fused=fused, itmax=steps, atol=0.0, rtol=0.0)
        ctx.sync()
        wall = time.perf_counter() - t0
        st = ws.stats
        assert st.niter == steps and not st.solved, (st.niter, st.status)
        return 1e3 * wall / st.niter, ws.last_path

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
    sb = A.spmv_bytes + At.spmv_bytes
    passes = {}
    for tag, per in PASS_BYTES.items():
        cnt, ms = prof[tag]
        passes[tag] = {"launches": cnt, "ms_per_launch": round(ms / max(cnt, 1), 4),
                       "TBps_on_%dn" % per: round(per * n / (ms / max(cnt, 1) * 1e-3) / 1e12, 3) if ms > 0 else None}
    out = {"operator": kind, "n1": n1, "steps": a.steps, "rounds": a.rounds, "paths": {f"path{f}": v for f, v in paths.items()},
           "ms_per_iter": {f"path{f}": round(min(v), 4) for f, v in times.items()},
           "ms_per_iter_all": {f"path{f}": [round(t, 4) for t in v] for f, v in times.items()},
           "event_split_path2": {"wall_ms_per_iter_with_brackets": round(wall, 4), "spmv_ms_per_iter": round(spmv_ms, 4),
                                 "rest_ms_per_iter": round(wall - spmv_ms, 4)},
           "passes_path2": passes,
           "algorithmic_GB_per_iter": {"path2": round((FUSED_BYTES * n + sb) / 1e9, 3), "path0": round((PRIMITIVE_BYTES * n + sb) / 1e9, 3)},
           "spmv_bytes_A_plus_At": sb}
    if 0 in times:
        pairs = [round(t2 / t0, 4) for t2, t0 in zip(times[2], times[0])]
        out["ratio_path2_over_path0_per_pair"] = pairs
        out["ratio_path2_over_path0"] = round(min(times[2]) / min(times[0]), 4)
        out["predicted_ratio_from_bytes"] = round((FUSED_BYTES * n + sb) / (PRIMITIVE_BYTES * n + sb), 4)
        out["path2_faster_in_every_pair"] = all(p < 1.0 for p in pairs)
    del ws
    if not a.no_siblings:                              # the yardstick: trilqr! on (A, b, c), path 2, the parent commit's code
        wt = K.TrilqrWorkspace(ctx, n, n)

        def run_trilqr(steps):
            ctx.sync(); t0 = time.perf_counter()
            K.trilqr_(wt, A, b, c, At=At, fused=2, itmax=steps, atol=0.0, rtol=0.0)
            ctx.sync()
            wall = time.perf_counter() - t0
            assert wt.stats.niter == steps and wt.last_path == 2, (wt.stats.niter, wt.stats.status, wt.last_path)
            return 1e3 * wall / steps

        run_trilqr(a.warmup)
        tt = [run_trilqr(a.steps) for _ in range(a.rounds)]
        ctx.set_option("profile_spmv", 1)
        ctx.profile_kernels()
        run_trilqr(a.steps)
        prof_t = ctx.profile_kernels()
        ctx.set_option("profile_spmv", 0)
        p3 = prof_t["trilqr_p3"][1] / max(prof_t["trilqr_p3"][0], 1)
        out["trilqr_path2_ms_per_iter"] = round(min(tt), 4)
        out["trilqr_path2_ms_per_iter_all"] = [round(t, 4) for t in tt]
        out["trilqr_p3_ms_per_launch_same_process"] = round(p3, 4)
        out["trilqr_p3_TBps_on_120n_same_process"] = round(120 * n / (p3 * 1e-3) / 1e12, 3)
        out["tricg_over_trilqr_path2"] = round(min(times[2]) / min(tt), 4)
        out["predicted_tricg_over_trilqr_from_bytes"] = round((FUSED_BYTES * n + sb) / (TRILQR_FUSED_BYTES * n + sb), 4)
        del wt
    lines.append(json.dumps(out))
    print(lines[-1], flush=True)
    del At, A, b, c
ctx.close()
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
