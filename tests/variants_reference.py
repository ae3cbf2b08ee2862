"""Test-side NumPy restatements of the opt-in recurrences of krylov.jl_amd/csrc/solvers.cpp, line by line, each with an injectable
`dot` (knorm(x) = sqrt(dot(x, x))) as in tests/qmr_reference.py.  Checkers, not product code: tests/test_variants_host.py pins them
to the oracle's cg! / gmres!, tests/test_gpu_variants.py compares the library's loops with them.

  cg_single_reduction   cg!(variant = 1): khip_cg_solve's setup, cgcg_start, cg_single_reduction_loop, cgcg_update_kernel
                        (csrc/blas1.hip) and the EPI_CGCG epilogue (csrc/solver_device.hpp)
  cg_pipelined          cg!(variant = 2): the same setup and epilogue, cg_pipelined_loop and pcg_update_kernel
  gmres_cgs2            gmres!(variant = 1): khip_gmres_solve with the CGS2 orthogonalisation

s-step gmres! (variant = 2) has none: its Hessenberg recovery is host code that no kernel pin reaches.
The kernels fuse each multiply-add; NumPy rounds the product first.  That difference is part of what the budgets of the GPU
tests measure (the sensitivity of a recurrence to the rounding of its dots bounds it from above in practice)."""
import math
from types import SimpleNamespace

import numpy as np

from bilq_reference import EPS, _op, fsum_dot, history_deviation, sym_givens  # noqa: F401  (re-exported for the tests)

SOLVED = "solution good enough given atol and rtol"
TIRED = "maximum number of iterations exceeded"
ZERO_RESIDUAL = "x is a zero-residual solution"
ZERO_CURVATURE = "zero curvature detected"
NOT_SPD = "The linear operator `A` or the preconditioner `M` is not symmetric positive definite."
INCONSISTENT = "found approximate least-squares solution"


def _cg_variant(pipelined, A, b, x0, atol, rtol, itmax, history, dot):
    mul = _op(A)
    b = np.asarray(b, dtype=np.float64)
    n = b.shape[0]
    st = SimpleNamespace(niter=0, solved=False, inconsistent=False, status="unknown", residuals=[], error=None, breakdown=False,
                         vectors={})

    def done(x):
        st.residuals = np.array(st.residuals)
        return x, st

    dx = None if x0 is None else np.asarray(x0, dtype=np.float64)
    x = np.zeros(n)                                                          # khip_cg_solve: x = 0
    r = b.copy() if dx is None else 1.0 * b + (-1.0) * mul(dx)               # r = b, or A dx then kaxpby!(1, b, -1, r)
    p = r.copy()                                                             # p = z = r (M = I)
    gamma = float(dot(r, r))
    if not gamma >= 0:
        st.error = st.status = NOT_SPD
        return done(x)
    rNorm = math.sqrt(gamma)
    if history:
        st.residuals.append(rNorm)
    if gamma == 0:
        st.solved, st.status = True, ZERO_RESIDUAL
        return done(x if dx is None else x + 1.0 * dx)
    it = 0
    if itmax == 0:
        itmax = 2 * n
    eps_tol = atol + rtol * rNorm
    solved = rNorm <= eps_tol
    tired = it >= itmax
    zero_curvature = False
    if not (solved or tired):
        s = np.zeros(n)                                                      # s = A p starts as 0 (beta_0 = 0)
        if pipelined:
            z = np.zeros(n)                                                  # z = A s, and p, start as 0 too
            p = np.zeros(n)
        w = mul(r)                                                           # w = A r ; (r.w, r.r)
        delta0 = float(dot(r, w))
        if not delta0 > 0:
            st.error = st.status = NOT_SPD                                   # KHIP_ERR_NUMERIC: the solve fails, x is left at 0
            st.vectors = dict(x=x, r=r, p=p, Ap=s, z=w)
            return done(x)
        alpha, beta = gamma / delta0, 0.0                                    # cgcg_start
        stopped = breakdown = False
        while it < itmax and not stopped:                                    # DeviceLoop::run: itmax iterations unless the state stops it
            if pipelined:
                q = mul(w)                                                   # (a) q = A w
                z = beta * z + q                                             # (b) pcg_update_kernel
                s = beta * s + w
                p = beta * p + r
                x = alpha * p + x
                r = (-alpha) * s + r
                w = (-alpha) * z + w
            else:
                p = beta * p + r                                             # cgcg_update_kernel
                s = beta * s + w
                x = alpha * p + x
                r = (-alpha) * s + r
                w = mul(r)                                                   # w = A r
            delta, gamma_next = float(dot(r, w)), float(dot(r, r))           # (r.w, r.r) in one reduction
            rNorm = math.sqrt(gamma_next)                                    # EPI_CGCG
            it += 1
            if history:
                st.residuals.append(rNorm)
            solved = rNorm <= eps_tol or rNorm + 1.0 <= 1.0
            beta_next = gamma_next / gamma
            with np.errstate(all="ignore"):
                denom = delta - float(np.float64(beta_next) * gamma_next / np.float64(alpha))
            breakdown = (not solved) and not (denom > 0.0)
            if solved or breakdown:
                stopped = True                                               # x, r already hold iterate k
                continue
            beta = beta_next
            alpha = gamma_next / denom
            gamma = gamma_next
        tired = it >= itmax
        st.breakdown = bool(breakdown)
        if breakdown and not solved:
            zero_curvature = st.inconsistent = True                          # as the cg! path reports it
        st.vectors = dict(x=x, r=r, p=p, Ap=s, z=w)
        if pipelined:
            st.vectors.update(pz=z, pq=q)
    status = "unknown"
    if solved:
        status = SOLVED
    if zero_curvature:
        status = ZERO_CURVATURE
    if tired:
        status = TIRED
    if dx is not None:
        x = 1.0 * dx + x
    st.vectors["x"] = x
    st.niter, st.solved, st.status = it, bool(solved), status
    return done(x)


def cg_single_reduction(A, b, x0=None, atol=math.sqrt(EPS), rtol=math.sqrt(EPS), itmax=0, history=True, dot=np.dot):
    """cg!(variant = 1), Chronopoulos & Gear: p = r + beta p, s = w + beta s, x += alpha p, r -= alpha s, w = A r, then
    (r.w, r.r).  Returns (x, stats); stats.vectors holds x, r, p, Ap (= s), z (= w) as khip_cg_vector names them; stats.error is
    the message of a refused solve (KHIP_ERR_NUMERIC) or None."""
    return _cg_variant(False, A, b, x0, atol, rtol, itmax, history, dot)


def cg_pipelined(A, b, x0=None, atol=math.sqrt(EPS), rtol=math.sqrt(EPS), itmax=0, history=True, dot=np.dot):
    """cg!(variant = 2), Ghysels & Vanroose: q = A w, then z = q + beta z, s = w + beta s, p = r + beta p, x += alpha p,
    r -= alpha s, w -= alpha z, then (r.w, r.r); the epilogue of variant 1.  stats.vectors also holds pz (= z) and pq (= q)."""
    return _cg_variant(True, A, b, x0, atol, rtol, itmax, history, dot)


def gmres_cgs2(A, b, x0=None, memory=20, restart=False, atol=math.sqrt(EPS), rtol=math.sqrt(EPS), itmax=0, history=True, dot=np.dot):
    """gmres!(variant = 1) with M = N = I: the loop of khip_gmres_solve (src/gmres.jl:121-384) with h = V'q, q -= V h applied
    twice, R = h + h2, Hbis = ||q||.  Returns (x, stats); stats.vectors holds x, w and the basis V of the last cycle."""
    mul = _op(A)
    norm = lambda v: math.sqrt(float(dot(v, v)))  # noqa: E731
    b = np.asarray(b, dtype=np.float64)
    n = b.shape[0]
    st = SimpleNamespace(niter=0, solved=False, inconsistent=False, status="unknown", residuals=[], vectors={}, inner_iter=0)

    def done(x):
        st.residuals = np.array(st.residuals)
        return x, st

    dx = None if x0 is None else np.asarray(x0, dtype=np.float64)
    x = np.zeros(n)                                                          # :155
    if dx is not None:
        w = 1.0 * b + (-1.0) * mul(dx)
        if restart:
            x = 1.0 * dx + x
    else:
        w = b.copy()
    beta = norm(w)                                                           # :166
    rNorm = beta
    if history:
        st.residuals.append(beta)
    eps_tol = atol + rtol * rNorm
    if beta == 0:
        st.solved, st.status = True, ZERO_RESIDUAL
        return done(x if dx is None else 1.0 * dx + x)
    mem = min(n, 20 if memory <= 0 else memory)                              # :188, memory = min(m, memory)
    npass = it = inner_iter = 0
    if itmax == 0:
        itmax = 2 * n
    inner_itmax = itmax
    btol = EPS ** 0.75                                                       # :195
    breakdown = inconsistent = False
    solved = rNorm <= eps_tol
    tired = it >= itmax
    V = [None] * mem
    xr = x
    while not (solved or tired or breakdown):
        c, s, z = [0.0] * mem, [0.0] * mem, [0.0] * mem
        R = []                                                               # R[k] = column k + 1 of the triangular factor
        if restart:
            xr = np.zeros(n)
            if npass >= 1:
                w = 1.0 * b + (-1.0) * mul(x)
        beta = norm(w)                                                       # :229
        z[0] = beta
        V[0] = w / rNorm                                                     # :231 divides by rNorm (the estimate), not beta
        npass += 1
        inner_iter = 0
        inner_tired = False
        while not (solved or inner_tired or breakdown):
            inner_iter += 1
            if not restart and inner_iter > mem:                             # :244-252
                s.append(0.0)
                c.append(0.0)
            q = mul(V[inner_iter - 1])                                       # :257
            k = inner_iter
            col = [0.0] * k
            for sweep in range(2):                                             # variant = 1: classical Gram-Schmidt, twice
                h = [float(dot(V[i], q)) for i in range(k)]                  # launch_multi_dot
                for i in range(k):                                           # launch_multi_axpy_dev: q -= h_i V_i, i = 0 .. k - 1
                    q = (-h[i]) * V[i] + q
                col = [h[i] if sweep == 0 else col[i] + h[i] for i in range(k)]  # R = h + h2
            Hbis = norm(q)
            for i in range(k - 1):                                           # :280-284
                Rtmp = c[i] * col[i] + s[i] * col[i + 1]
                col[i + 1] = s[i] * col[i] - c[i] * col[i + 1]
                col[i] = Rtmp
            c[k - 1], s[k - 1], col[k - 1] = sym_givens(col[k - 1], Hbis)    # :289
            R.append(col)
            zeta_next = s[k - 1] * z[k - 1]                                  # :292-293
            z[k - 1] = c[k - 1] * z[k - 1]
            rNorm = abs(zeta_next)
            if history:
                st.residuals.append(rNorm)
            resid_decrease_mach = rNorm + 1.0 <= 1.0
            resid_decrease_lim = rNorm <= eps_tol
            breakdown = Hbis <= btol
            solved = resid_decrease_lim or resid_decrease_mach
            inner_tired = inner_iter >= (min(mem, inner_itmax) if restart else inner_itmax)
            if not (solved or inner_tired or breakdown):
                if not restart and inner_iter >= mem:                        # :319-324
                    if len(V) <= inner_iter:
                        V.append(None)
                    if len(z) <= inner_iter:
                        z.append(0.0)
                V[inner_iter] = q / Hbis                                     # :325
                z[inner_iter] = zeta_next
        y = z                                                                # :331-345
        for i in range(inner_iter, 0, -1):
            for j in range(inner_iter, i, -1):
                y[i - 1] = y[i - 1] - R[j - 1][i - 1] * y[j - 1]
            if abs(R[i - 1][i - 1]) <= btol:
                y[i - 1] = 0.0
                inconsistent = True
            else:
                y[i - 1] = y[i - 1] / R[i - 1][i - 1]
        for i in range(inner_iter):                                          # :348-350, khip_multi_axpy in the order i = 0 ..
            xr = y[i] * V[i] + xr
        if restart:
            x = 1.0 * xr + x                                                 # :355
        else:
            x = xr
        inner_itmax -= inner_iter
        it += inner_iter
        tired = it >= itmax
    status = "unknown"
    if tired:
        status = TIRED
    if solved:
        status = SOLVED
    if inconsistent:
        status = INCONSISTENT
    if dx is not None and not restart:
        x = 1.0 * dx + x
    st.vectors = dict(x=x, w=w, V=[v for v in V if v is not None])
    st.niter, st.solved, st.inconsistent, st.status, st.inner_iter = it, bool(solved), bool(inconsistent), status, inner_iter
    return done(x)
