#!/usr/bin/env python3
"""trilqr! on the 512^3 Poisson operator and on kron_unsymmetric(256) with c = A' b ≠ b (A' built by transpose()): ms per iteration of
the device-resident loop (path 2) and of the primitive sequence (path 0), alternated over --rounds pairs of --steps iterations after
a warm-up (atol = rtol = 0 and itmax = steps: every run does the full count with both sides unsolved; the transfer to USYMCG is on,
its test never fires at a zero tolerance), and, in the same process, what trilqr! replaces: usymlq! on (A, b, c) followed by usymqr!
on (A', c, b), both on their path 2 (trilqr! moves 224 n bytes per iteration beside two products, its primitive sequence 368 n;
usymlq! 176 n and usymqr! 184 n, each beside two products of its own).
One more path-2 solve runs with the HIP-event brackets on (khip_profile_kernels): the products and each of the three passes, as ms per
launch and as TB/s on the pass's bytes (P1 56 n, P2 48 n, P3 120 n; the lighter P1 and P3 of the first iterations are in the mean).
Prints one JSON line per operator; --out also writes them to a file (profiles/trilqr_bench.json).

    python tools/bench_trilqr.py --out profiles/trilqr_bench.json
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

PASS_BYTES = {"ssy_p1": 56, "ssy_p2": 48, "trilqr_p3": 120}      # per entry of a vector
FUSED_BYTES, PRIMITIVE_BYTES, USYMLQ_FUSED_BYTES, USYMQR_FUSED_BYTES = 224, 368, 176, 184
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
    c = At.matvec(b)                                   # c = A' b: not b, also where A is symmetric
    ws = K.TrilqrWorkspace(ctx, n, n)

    def run(fused, steps):
        ctx.sync(); t0 = time.perf_counter()
        K.trilqr_(ws, A, b, c, At=At, fused=fused, itmax=steps, atol=0.0, rtol=0.0)
        ctx.sync()
        wall = time.perf_counter() - t0
        st = ws.stats
        assert st.niter == steps and not st.solved_primal and not st.solved_dual, (st.niter, st.status)
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
    if not a.no_siblings:                              # what trilqr! replaces: usymlq! on (A, b, c), then usymqr! on (A', c, b); path 2 each
        wl, wq = K.UsymlqWorkspace(ctx, n, n), K.UsymqrWorkspace(ctx, n, n)

        def run_usymlq(steps):
            ctx.sync(); t0 = time.perf_counter()
            K.usymlq_(wl, A, b, c, At=At, fused=2, itmax=steps, atol=0.0, rtol=0.0)
            ctx.sync()
            wall = time.perf_counter() - t0
            assert wl.stats.niter == steps and wl.last_path == 2, (wl.stats.niter, wl.stats.status, wl.last_path)
            return 1e3 * wall / steps

        def run_usymqr(steps):
            ctx.sync(); t0 = time.perf_counter()
            K.usymqr_(wq, At, c, b, At=A, fused=2, itmax=steps, atol=0.0, rtol=0.0)
            ctx.sync()
            wall = time.perf_counter() - t0
            assert wq.stats.niter == steps and wq.last_path == 2, (wq.stats.niter, wq.stats.status, wq.last_path)
            return 1e3 * wall / steps

        run_usymlq(a.warmup); run_usymqr(a.warmup)
        tl, tq = [], []
        for _ in range(a.rounds):
            tl.append(run_usymlq(a.steps)); tq.append(run_usymqr(a.steps))
        ctx.set_option("profile_spmv", 1)
        ctx.profile_kernels()
        run_usymlq(a.steps)
        prof_l = ctx.profile_kernels()
        ctx.set_option("profile_spmv", 0)
        out["usymlq_path2_ms_per_iter"] = round(min(tl), 4)
        out["usymlq_path2_ms_per_iter_all"] = [round(t, 4) for t in tl]
        out["usymqr_path2_ms_per_iter"] = round(min(tq), 4)
        out["usymqr_path2_ms_per_iter_all"] = [round(t, 4) for t in tq]
        out["usymlq_p3_ms_per_launch_same_session"] = round(prof_l["usymlq_p3"][1] / max(prof_l["usymlq_p3"][0], 1), 4)
        out["usymlq_p3_TBps_on_72n_same_session"] = round(72 * n / (prof_l["usymlq_p3"][1] / max(prof_l["usymlq_p3"][0], 1) * 1e-3) / 1e12, 3)
        out["trilqr_over_usymlq_plus_usymqr_path2"] = round(min(times[2]) / (min(tl) + min(tq)), 4)
        out["predicted_trilqr_over_pair_from_bytes"] = round((FUSED_BYTES * n + sb) / ((USYMLQ_FUSED_BYTES + USYMQR_FUSED_BYTES) * n + 2 * sb), 4)
        del wl, wq
    lines.append(json.dumps(out))
    print(lines[-1], flush=True)
    del At, A, b, c
ctx.close()
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
