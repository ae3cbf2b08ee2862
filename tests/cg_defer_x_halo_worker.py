"""One process, ONE RCCL rank that exchanges its halo with ITSELF (test hook khip_test_set_halo_self, as tests/self_halo_worker.py):
cg! on a periodic slab of the 7-point grid with x updated every second iteration (ctx option cg_defer_x = 1) against every
iteration (0) -- on a row-partitioned run the halo exchange of every second product packs from the second direction buffer --
and against the same periodic operator as a plain single-GPU CSR.  Driven by tests/test_gpu_cg_defer_x.py.
argv: n1 k0 k1 out.json"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import krylov_jl_amd as K  # noqa: E402


def main():
    n1, k0, k1, out = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    plane = n1 * n1
    r0, r1 = k0 * plane, k1 * plane
    m = r1 - r0
    ctx = K.Context(0)
    ctx.test_set_halo_self(1)                    # before the communicator: it splits off the halo communicator for one rank too
    ctx.comm_init(0, 1, K.Context.comm_unique_id())
    A = K.CsrMatrix.stencil(ctx, "poisson", n1, rows=(r0, r1), distributed=True)
    res = {"n_ghost": A.halo_info[1], "cases": {}}
    ctx2 = K.Context(0)
    rp, col, val = K.gen_stencil_arrays(ctx2, "poisson", n1, rows=(r0, r1))
    P = K.CsrMatrix.from_host(ctx2, rp, ((col.astype(np.int64) - r0) % m).astype(np.int32), val, (m, m))
    bh = np.random.default_rng(5).standard_normal(m)
    b, b2 = ctx.array(bh), ctx2.array(bh)
    for itmax in (3, 6, 0):                       # a flush, an even count, convergence
        kw = dict(history=True, fused=2, atol=0.0, rtol=0.0 if itmax else 1e-10, itmax=itmax if itmax else 60)
        st = []
        for defer in (0, 1):
            ctx.set_option("cg_defer_x", defer)
            ws = K.CgWorkspace(ctx, m, m)
            K.cg_(ws, A, b, **kw)
            st.append(({k: ws.vector(k).to_host() for k in ("x", "r", "p", "Ap")}, ws.stats, ws.last_path))
        ws2 = K.CgWorkspace(ctx2, m, m)
        K.cg_(ws2, P, b2, **kw)
        h1, h2 = st[1][1].residuals, ws2.stats.residuals
        eq = {k: bool(np.array_equal(st[0][0][k], st[1][0][k])) for k in ("x", "r", "p", "Ap")}
        eq["residuals"] = bool(np.array_equal(st[0][1].residuals, st[1][1].residuals))
        res["cases"][str(itmax)] = {"equal": eq, "niter": [int(s[1].niter) for s in st], "status": [s[1].status for s in st],
                                    "last_path": [int(s[2]) for s in st], "plain_niter": int(ws2.stats.niter),
                                    "max_rel_dev_plain": float(np.max(np.abs(h1 - h2) / h2)) if len(h1) == len(h2) else None}
    json.dump(res, open(out, "w"))
    print(json.dumps(res))
    os._exit(0)           # skip the communicator teardown: nothing to learn from it here


if __name__ == "__main__":
    main()
