#!/usr/bin/env python3
"""trimr! on the 512^3 Poisson operator (c = A' b + ones) and on kron_unsymmetric(256) (c = A' b), A' built by transpose(): ms per
iteration of the device-resident loop (path 2) and of the primitive sequence (path 0), alternated over --rounds pairs of --steps iterations after a
warm-up (atol = rtol = 0 and itmax = steps: every run does the full count), and, in the same process, tricg! on its path 2 as the
yardstick: the code of the parent commit on the same driver (trimr! moves 280 n bytes per iteration beside two products, its
primitive sequence 496 n; tricg! 248 n).
--rounds more path-2 solves of trimr! and of tricg!, alternated, run with the HIP-event brackets on (khip_profile_kernels): the
products and each of the three passes, as ms per launch and as TB/s on the pass's bytes (P1 56 n, P2 48 n, trimr!'s P3 176 n,
tricg!'s P3 144 n; the lighter P1 and P3 of the first iterations are in the mean).  trimr!'s P3 does four FP64 divisions per
element where tricg!'s does none: its per-byte rate is held against tricg_p3's of the same round, and the margin is the spread of
tricg_p3's rate over the rounds.
Prints one JSON line per operator; --out also writes them to a file (profiles/trimr_bench.json).

    python tools/bench_trimr.py --out profiles/trimr_bench.json
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

PASS_BYTES = {"ssy_p1": 56, "ssy_p2": 48, "trimr_p3": 176}       # per entry of a vector
FUSED_BYTES, PRIMITIVE_BYTES, TRICG_FUSED_BYTES, TRICG_P3_BYTES = 280, 496, 248, 144
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
    if kind == "poisson":                              # A symmetric: c = A b has the solution x = b, y = 0 in span{v1}, and trimr! stops
        K.kaxpy_(n, 1.0, x1, c)                        # after two iterations; c = A' b + ones runs the full count
    del x1
    ws = K.TrimrWorkspace(ctx, n, n)
    wc = K.TricgWorkspace(ctx, n, n)

    def run(fused, steps):
        ctx.sync(); t0 = time.perf_counter()
        K.trimr_(ws, A, b, c, At=At, fused=fused, itmax=steps, atol=0.0, rtol=0.0)
        ctx.sync()
        wall = time.perf_counter() - t0
        st = ws.stats
        assert st.niter == steps and not st.solved, (st.niter, st.status)
        return 1e3 * wall / st.niter, ws.last_path

    def run_tricg(steps):
        ctx.sync(); t0 = time.perf_counter()
        K.tricg_(wc, A, b, c, At=At, fused=2, itmax=steps, atol=0.0, rtol=0.0)
        ctx.sync()
        wall = time.perf_counter() - t0
        assert wc.stats.niter == steps and wc.last_path == 2, (wc.stats.niter, wc.stats.status, wc.last_path)
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
    run_tricg(a.warmup)
    times, paths, tt = {f: [] for f in legs}, {}, []
    for _ in range(a.rounds):
        for f in legs:
            t, paths[f] = run(f, a.steps)
            times[f].append(t)
        tt.append(run_tricg(a.steps))
    # the brackets, alternated: per round one path-2 solve of each solver
    per_launch = {tag: [] for tag in PASS_BYTES}
    tricg_p3, spmv, walls = [], [], []
    for _ in range(a.rounds):
        wall, prof = bracketed(lambda: run(2, a.steps)[0])
        walls.append(wall)
        spmv.append(prof["spmv"][1] / a.steps)
        for tag in PASS_BYTES:
            cnt, ms = prof[tag]
            assert cnt == a.steps, (tag, cnt)
            per_launch[tag].append(ms / cnt)
        _, prof_c = bracketed(lambda: run_tricg(a.steps))
        assert prof_c["tricg_p3"][0] == a.steps
        tricg_p3.append(prof_c["tricg_p3"][1] / a.steps)
    tbps = lambda per, ms: per * n / (ms * 1e-3) / 1e12  # noqa: E731
    passes = {tag: {"launches_per_solve": a.steps, "ms_per_launch": round(min(v), 4), "ms_per_launch_all": [round(t, 4) for t in v],
                    "TBps_on_%dn" % PASS_BYTES[tag]: round(tbps(PASS_BYTES[tag], min(v)), 3),
                    "TBps_all": [round(tbps(PASS_BYTES[tag], t), 3) for t in v]} for tag, v in per_launch.items()}
    sb = A.spmv_bytes + At.spmv_bytes
    spmv_ms = min(spmv)
    out = {"operator": kind, "n1": n1, "c": "A'b + ones" if kind == "poisson" else "A'b", "steps": a.steps, "rounds": a.rounds,
           "paths": {f"path{f}": v for f, v in paths.items()},
           "ms_per_iter": {f"path{f}": round(min(v), 4) for f, v in times.items()},
           "ms_per_iter_all": {f"path{f}": [round(t, 4) for t in v] for f, v in times.items()},
           "event_split_path2": {"wall_ms_per_iter_with_brackets": round(min(walls), 4), "spmv_ms_per_iter": round(spmv_ms, 4),
                                 "rest_ms_per_iter": round(min(walls) - spmv_ms, 4)},
           "passes_path2": passes,
           "algorithmic_GB_per_iter": {"path2": round((FUSED_BYTES * n + sb) / 1e9, 3), "path0": round((PRIMITIVE_BYTES * n + sb) / 1e9, 3)},
           "spmv_bytes_A_plus_At": sb}
    if 0 in times:
        pairs = [round(t2 / t0, 4) for t2, t0 in zip(times[2], times[0])]
        out["ratio_path2_over_path0_per_pair"] = pairs
        out["ratio_path2_over_path0"] = round(min(times[2]) / min(times[0]), 4)
        out["predicted_ratio_from_bytes"] = round((FUSED_BYTES * n + sb) / (PRIMITIVE_BYTES * n + sb), 4)
        # the same prediction with the products at their MEASURED time and the vector bytes at P3's measured rate
        rate = PASS_BYTES["trimr_p3"] * n / min(per_launch["trimr_p3"])          # bytes per ms
        out["predicted_ratio_with_measured_spmv"] = round((spmv_ms + FUSED_BYTES * n / rate) / (spmv_ms + PRIMITIVE_BYTES * n / rate), 4)
        out["path2_faster_in_every_pair"] = all(p < 1.0 for p in pairs)
    rates_c = [tbps(TRICG_P3_BYTES, t) for t in tricg_p3]
    rates_m = [tbps(PASS_BYTES["trimr_p3"], t) for t in per_launch["trimr_p3"]]
    out["tricg_path2_ms_per_iter"] = round(min(tt), 4)
    out["tricg_path2_ms_per_iter_all"] = [round(t, 4) for t in tt]
    out["tricg_p3_ms_per_launch_same_process"] = [round(t, 4) for t in tricg_p3]
    out["tricg_p3_TBps_on_144n_same_process"] = [round(r, 3) for r in rates_c]
    out["tricg_p3_TBps_spread"] = round(max(rates_c) - min(rates_c), 3)
    out["trimr_p3_over_tricg_p3_per_byte_rate_per_round"] = [round(m / c_, 4) for m, c_ in zip(rates_m, rates_c)]
    out["trimr_p3_rate_below_tricg_p3_by_more_than_its_spread"] = bool(max(rates_m) < min(rates_c) - (max(rates_c) - min(rates_c)))
    out["trimr_over_tricg_path2"] = round(min(times[2]) / min(tt), 4)
    out["predicted_trimr_over_tricg_from_bytes"] = round((FUSED_BYTES * n + sb) / (TRICG_FUSED_BYTES * n + sb), 4)
    del ws, wc
    lines.append(json.dumps(out))
    print(lines[-1], flush=True)
    del At, A, b, c
ctx.close()
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
