#!/usr/bin/env python3
"""usymlqr! (ls = ln = true) on the 512^3 Poisson operator (c = A' b + ones) and on kron_unsymmetric(256) (c = A' b), A' built by
transpose(): ms per iteration of the device-resident loop (path 2) and of the primitive sequence (path 0), alternated over --rounds
pairs of --steps iterations after a warm-up (atol = rtol = 0 and itmax = steps: every run does the full count with both sides
active), beside the ratio the byte counts predict (usymlqr! moves 256 n bytes per iteration beside two products, its primitive
sequence 416 n; the products at the handle's spmv_bytes).
--rounds more path-2 solves of usymlqr! and of trimr!, alternated, run with the HIP-event brackets on (khip_profile_kernels): the
products and each of the three passes, as ms per launch and as TB/s on the pass's bytes (P1 56 n, P2 48 n, usymlqr!'s P3 152 n,
trimr!'s P3 176 n; the lighter P1 and P3 of the first iterations are in the mean).  usymlqr_p3's per-byte rate is held against
trimr_p3's of the same round; the margin is the spread of trimr_p3's rate over the rounds.
Prints one JSON line per operator; --out also writes them to a file.

    python tools/bench_usymlqr.py --out profiles/usymlqr_bench_ab.json
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
ap.add_argument("--out", default=None)
a = ap.parse_args()

PASS_BYTES = {"ssy_p1": 56, "ssy_p2": 48, "usymlqr_p3": 152}     # per entry of a vector
FUSED_BYTES, PRIMITIVE_BYTES, TRIMR_P3_BYTES = 256, 416, 176
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
    c = At.matvec(b)                                   # c = A' b
    if kind == "poisson":                              # A symmetric: with c = A b the two Krylov spaces coincide; c = A' b + ones
        K.kaxpy_(n, 1.0, x1, c)                        # keeps them apart, as in tools/bench_trimr.py
    del x1
    ws = K.UsymlqrWorkspace(ctx, n, n)
    wm = K.TrimrWorkspace(ctx, n, n)

    def run(fused, steps):
        ctx.sync(); t0 = time.perf_counter()
        K.usymlqr_(ws, A, b, c, At=At, fused=fused, itmax=steps, atol=0.0, rtol=0.0)
        ctx.sync()
        wall = time.perf_counter() - t0
        st = ws.stats
        assert st.niter == steps and not st.solved, (st.niter, st.status)
        return 1e3 * wall / st.niter, ws.last_path

    def run_trimr(steps):
        ctx.sync(); t0 = time.perf_counter()
        K.trimr_(wm, A, b, c, At=At, fused=2, itmax=steps, atol=0.0, rtol=0.0)
        ctx.sync()
        wall = time.perf_counter() - t0
        assert wm.stats.niter == steps and wm.last_path == 2, (wm.stats.niter, wm.stats.status, wm.last_path)
        return 1e3 * wall / steps

    def bracketed(solve):
        ctx.set_option("profile_spmv", 1)
        ctx.profile_kernels()
        wall = solve()
        prof = ctx.profile_kernels()
        ctx.set_option("profile_spmv", 0)
        return wall, prof

    legs = (2,) if a.no_path0 else (2, 0)
    for f in legs:
        run(f, a.warmup)
    run_trimr(a.warmup)
    times, paths, tt = {f: [] for f in legs}, {}, []
    for _ in range(a.rounds):
        for f in legs:
            t, paths[f] = run(f, a.steps)
            times[f].append(t)
        tt.append(run_trimr(a.steps))
    # the brackets, alternated: per round one path-2 solve of each solver
    per_launch = {tag: [] for tag in PASS_BYTES}
    trimr_p3, spmv, walls = [], [], []
    for _ in range(a.rounds):
        wall, prof = bracketed(lambda: run(2, a.steps)[0])
        walls.append(wall)
        spmv.append(prof["spmv"][1] / a.steps)
        for tag in PASS_BYTES:
            cnt, ms = prof[tag]
            assert cnt == a.steps, (tag, cnt)
            per_launch[tag].append(ms / cnt)
        _, prof_m = bracketed(lambda: run_trimr(a.steps))
        assert prof_m["trimr_p3"][0] == a.steps
        trimr_p3.append(prof_m["trimr_p3"][1] / a.steps)
    tbps = lambda per, ms: per * n / (ms * 1e-3) / 1e12  # noqa: E731
    passes = {tag: {"launches_per_solve": a.steps, "ms_per_launch": round(min(v), 4), "ms_per_launch_all": [round(t, 4) for t in v],
                    "TBps_on_%dn" % PASS_BYTES[tag]: round(tbps(PASS_BYTES[tag], min(v)), 3),
                    "TBps_all": [round(tbps(PASS_BYTES[tag], t), 3) for t in v]} for tag, v in per_launch.items()}
    sb = A.spmv_bytes + At.spmv_bytes
    spmv_ms = min(spmv)
    out = {"operator": kind, "n1": n1, "c": "A'b + ones" if kind == "poisson" else "A'b", "ls": True, "ln": True, "steps": a.steps,
           "rounds": a.rounds, "paths": {f"path{f}": v for f, v in paths.items()},
           "ms_per_iter": {f"path{f}": round(min(v), 4) for f, v in times.items()},
           "ms_per_iter_all": {f"path{f}": [round(t, 4) for t in v] for f, v in times.items()},
           "event_split_path2": {"wall_ms_per_iter_with_brackets": round(min(walls), 4), "spmv_ms_per_iter": round(spmv_ms, 4),
                                 "rest_ms_per_iter": round(min(walls) - spmv_ms, 4)},
           "passes_path2": passes,
           "algorithmic_GB_per_iter": {"path2": round((FUSED_BYTES * n + sb) / 1e9, 3), "path0": round((PRIMITIVE_BYTES * n + sb) / 1e9, 3)},
           "spmv_bytes_A_plus_At": sb}
    if 0 in times:
        pairs = [round(t2 / t0, 4) for t2, t0 in zip(times[2], times[0])]
        spread = max(pairs) - min(pairs)
        out["ratio_path2_over_path0_per_pair"] = pairs
        out["ratio_path2_over_path0"] = round(min(times[2]) / min(times[0]), 4)
        out["ratio_spread_over_pairs"] = round(spread, 4)
        out["predicted_ratio_from_bytes"] = round((FUSED_BYTES * n + sb) / (PRIMITIVE_BYTES * n + sb), 4)
        # the same prediction with the products at their MEASURED time and the vector bytes at P3's measured rate
        rate = PASS_BYTES["usymlqr_p3"] * n / min(per_launch["usymlqr_p3"])      # bytes per ms
        out["predicted_ratio_with_measured_spmv"] = round((spmv_ms + FUSED_BYTES * n / rate) / (spmv_ms + PRIMITIVE_BYTES * n / rate), 4)
        out["path2_faster_in_every_pair"] = all(p < 1.0 for p in pairs)
    rates_m = [tbps(TRIMR_P3_BYTES, t) for t in trimr_p3]
    rates_u = [tbps(PASS_BYTES["usymlqr_p3"], t) for t in per_launch["usymlqr_p3"]]
    out["trimr_path2_ms_per_iter"] = round(min(tt), 4)
    out["trimr_path2_ms_per_iter_all"] = [round(t, 4) for t in tt]
    out["trimr_p3_ms_per_launch_same_process"] = [round(t, 4) for t in trimr_p3]
    out["trimr_p3_TBps_on_176n_same_process"] = [round(r, 3) for r in rates_m]
    out["trimr_p3_TBps_spread"] = round(max(rates_m) - min(rates_m), 3)
    out["usymlqr_p3_TBps_on_152n"] = [round(r, 3) for r in rates_u]
    out["usymlqr_p3_over_trimr_p3_per_byte_rate_per_round"] = [round(u / m_, 4) for u, m_ in zip(rates_u, rates_m)]
    out["usymlqr_p3_rate_below_trimr_p3_by_more_than_its_spread"] = bool(max(rates_u) < min(rates_m) - (max(rates_m) - min(rates_m)))
    del ws, wm
    lines.append(json.dumps(out))
    print(lines[-1], flush=True)
    del At, A, b, c
ctx.close()
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
