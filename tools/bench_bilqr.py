#!/usr/bin/env python3
"""bilqr! on the 512^3 Poisson operator and on kron_unsymmetric(256) (A' built by transpose()): ms per iteration of the
device-resident loop (path 2) and of the primitive sequence (path 0), and, in the same process, of bilq! path 2 plus qmr! path 2 on
A' -- what a user pays today for the same pair of solutions -- alternated over --rounds rounds of --steps iterations after a warm-up
(atol = rtol = 0 and itmax = steps: every run does the full count, both sides of bilqr! stay active).  bilqr! moves 224 n bytes per
iteration beside the two products, its primitive sequence 400 n, bilq! and qmr! together 176 n + 184 n beside four products.
Prints one JSON line per operator; --out also writes them to a file (profiles/bilqr_bench.json).

    python tools/bench_bilqr.py --out profiles/bilqr_bench.json
    rocprofv3 --kernel-trace --stats ... -- python tools/bench_bilqr.py --operators poisson:512 --rounds 1 --no-path0 --no-pair     (per-kernel times)
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
ap.add_argument("--no-pair", action="store_true")
ap.add_argument("--out", default=None)
a = ap.parse_args()

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
    c = At.matvec(x1)                                  # c = A' ones
    del x1
    ws = K.BilqrWorkspace(ctx, n, n)
    wb = wq = None
    if not a.no_pair:
        wb = K.BilqWorkspace(ctx, n, n)
        wq = K.QmrWorkspace(ctx, n, n)

    def run(fused, steps):
        ctx.sync(); t0 = time.perf_counter()
        K.bilqr_(ws, A, b, c, At=At, fused=fused, itmax=steps, atol=0.0, rtol=0.0)
        ctx.sync()
        st = ws.stats
        assert st.niter == steps and ws.last_path == fused, (st.niter, st.status, ws.last_path)
        return 1e3 * (time.perf_counter() - t0) / st.niter

    def run_pair(steps):                               # x of A x = b by bilq!, y of A' y = c by qmr! on A'
        ctx.sync(); t0 = time.perf_counter()
        K.bilq_(wb, A, b, c=c, At=At, fused=2, itmax=steps, atol=0.0, rtol=0.0)
        K.qmr_(wq, At, c, c=b, At=A, fused=2, itmax=steps, atol=0.0, rtol=0.0)
        ctx.sync()
        assert wb.stats.niter == steps and wq.stats.niter == steps and wb.last_path == 2 and wq.last_path == 2
        return 1e3 * (time.perf_counter() - t0) / steps

    legs = [2] + ([] if a.no_path0 else [0]) + ([] if a.no_pair else ["pair"])
    go = lambda leg, steps: run_pair(steps) if leg == "pair" else run(leg, steps)  # noqa: E731
    for leg in legs:
        go(leg, a.warmup)
    times = {leg: [] for leg in legs}
    for _ in range(a.rounds):
        for leg in legs:
            times[leg].append(go(leg, a.steps))
    sb = A.spmv_bytes + At.spmv_bytes
    name = lambda leg: "bilq_plus_qmr_path2" if leg == "pair" else f"path{leg}"  # noqa: E731
    out = {"operator": kind, "n1": n1, "steps": a.steps, "rounds": a.rounds,
           "ms_per_iter": {name(leg): round(min(v), 4) for leg, v in times.items()},
           "ms_per_iter_all": {name(leg): [round(t, 4) for t in v] for leg, v in times.items()},
           "algorithmic_GB_per_iter": {"path2": round((224 * n + sb) / 1e9, 3), "path0": round((400 * n + sb) / 1e9, 3),
                                       "bilq_plus_qmr_path2": round((360 * n + 2 * sb) / 1e9, 3)},
           "spmv_bytes_A_plus_At": sb}
    if 0 in times:
        pairs = [round(t2 / t0, 4) for t2, t0 in zip(times[2], times[0])]
        out["ratio_path2_over_path0_per_pair"] = pairs
        out["predicted_path2_over_path0_from_bytes"] = round((224 * n + sb) / (400 * n + sb), 4)
        out["path2_faster_than_path0_in_every_pair"] = all(p < 1.0 for p in pairs)
    if "pair" in times:
        pairs = [round(t2 / tp, 4) for t2, tp in zip(times[2], times["pair"])]
        out["ratio_path2_over_bilq_plus_qmr_per_pair"] = pairs
        out["predicted_path2_over_bilq_plus_qmr_from_bytes"] = round((224 * n + sb) / (360 * n + 2 * sb), 4)
        out["path2_faster_than_bilq_plus_qmr_in_every_pair"] = all(p < 1.0 for p in pairs)
    lines.append(json.dumps(out))
    print(lines[-1], flush=True)
    del ws, wb, wq, At, A, b, c
ctx.close()
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
