"""One process, ONE RCCL rank: the device-side cross-rank combine of the compensated dots (csrc/blas1.hip combine_kernel, reached
through comm_allreduce_dd_device) on the device-resident cg! loop (fused = 2), against the same loop on a context without a
communicator.  With one rank the all-gather returns the rank's own (hi, lo) partial and the combine folds it with TwoSum from
0: finite scalars keep their bits, and a partial whose hi overflowed must stay +Inf rather than become NaN.
Driven by tests/test_gpu_reduction_exact.py (own process, as tests/self_halo_worker.py).  argv: n1 out.json"""
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import krylov_jl_amd as K  # noqa: E402


def overflow_rhs(n1):
    """b = a (u_low + sqrt(t) u_high) on get_div_grad(n1, n1, n1), u_low / u_high its smallest / largest Dirichlet eigenvectors
    (unit norm), t = lambda_min / 12: b . b = 1e307 and p . Ap = b . Ab stay finite, but the first CG step's residual
    r = b - (b.b / b.Ab) A b has r . r of about 1e309 -- a sum of finite squares that overflows (every one of them < 1e306)."""
    i = np.arange(1, n1 + 1)
    lo, hi = np.sin(np.pi * i / (n1 + 1)), np.sin(n1 * np.pi * i / (n1 + 1))
    ul = np.einsum("i,j,k->ijk", lo, lo, lo).ravel()
    uh = np.einsum("i,j,k->ijk", hi, hi, hi).ravel()
    ul /= np.linalg.norm(ul)
    uh /= np.linalg.norm(uh)
    lam_min = 3.0 * (2.0 - 2.0 * np.cos(np.pi / (n1 + 1)))
    return math.sqrt(1e307) * (ul + math.sqrt(lam_min / 12.0) * uh)


def solve(ctx, A, b_host, fused):
    n = b_host.size
    ws = K.CgWorkspace(ctx, n, n)
    err = ""
    try:
        K.cg_(ws, A, ctx.array(b_host), history=True, fused=fused, itmax=40, atol=0.0, rtol=1e-10)
    except K.KhipError as e:          # the overflowing case ends in the "not symmetric positive definite" test (NaN after Inf)
        err = str(e)
    st = ws.stats
    return dict(niter=int(st.niter), status=str(st.status), error=err, hist=[float(v) for v in st.residuals],
                path=int(ws.last_path))


def main():
    n1, out = int(sys.argv[1]), sys.argv[2]
    n = n1 ** 3
    res = {}
    ctx = K.Context(0)
    ctx.comm_init(0, 1, K.Context.comm_unique_id())
    info = ctx.comm_info()
    res["rccl_ranks"], res["local_backend"] = info["rccl_ranks"], info["local_backend"]
    A = K.CsrMatrix.stencil(ctx, "poisson", n1, rows=(0, n), distributed=True)
    ctx2 = K.Context(0)                                  # no communicator: the finish kernel's scalars go straight to the epilogue
    P = K.CsrMatrix.stencil(ctx2, "poisson", n1)
    b = np.linspace(0.5, 2.0, n)
    # the combine runs: its launches are bracketed (khip_profile_kernels "dot_allgather_combine")
    ctx.set_option("profile_spmv", 1)
    ctx.profile_kernels()
    res["probe"] = solve(ctx, A, b, 2)
    res["combine_launches"] = ctx.profile_kernels()["dot_allgather_combine"][0]
    ctx.set_option("profile_spmv", 0)
    for name, rhs in (("finite", b), ("overflow", overflow_rhs(n1))):
        for fused in (2, 1):
            res[f"{name}_comm_f{fused}"] = solve(ctx, A, rhs, fused)
            res[f"{name}_plain_f{fused}"] = solve(ctx2, P, rhs, fused)
    json.dump(res, open(out, "w"))
    print(json.dumps(res)[:4000])
    os._exit(0)           # skip the communicator teardown: nothing to learn from it here


if __name__ == "__main__":
    main()
