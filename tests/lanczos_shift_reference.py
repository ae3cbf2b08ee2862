"""Test-side NumPy restatement of cg_lanczos_shift! (src/cg_lanczos_shift.jl:107-284), line by line, with an injectable `dot`
for kdotr (np.dot, or math.fsum for exactly summed dots) and knorm = sqrt(dot(x, x)).  A checker, not product code:
tests/test_lanczos_shift_host.py and tests/test_gpu_lanczos_shift.py compare the library's three loops with it."""
import math
import time
from types import SimpleNamespace

import numpy as np

EPS = np.finfo(np.float64).eps


def cg_lanczos_shift(A, b, shifts, M=None, check_curvature=False, atol=math.sqrt(EPS), rtol=math.sqrt(EPS), itmax=0,
                     timemax=math.inf, history=True, callback=None, verbose=0, iostream=None, dot=np.dot, vectors=True):
    """A, M: callables v -> A v (M: v -> M⁻¹ v, symmetric positive definite) or objects with `@`.  callback(ws) sees a namespace
    with x (list), rNorms, converged, not_cv, stats.  vectors = False skips the x_i / p_i updates, which no scalar depends on
    (histories of large cases).  Returns (x, stats, ws)."""
    start = time.perf_counter()
    mul = A if callable(A) else (lambda v: A @ v)
    prec = None if M is None else (M if callable(M) else (lambda v: M @ v))
    b = np.asarray(b, dtype=np.float64)
    shifts = [float(s) for s in shifts]
    n, nshifts = b.shape[0], len(shifts)
    MisI = prec is None
    out = iostream.write if iostream is not None else None
    if verbose > 0 and out:
        out("CG-LANCZOS-SHIFT: system of %d equations in %d variables with %d shifts\n" % (n, n, nshifts))
    st = SimpleNamespace(niter=0, solved=False, status="unknown", residuals=[[] for _ in range(nshifts)],
                         indefinite=[False] * nshifts)
    x = [np.zeros(n) for _ in range(nshifts)]
    Mv = b.copy()
    v = Mv if MisI else prec(Mv)
    beta = math.sqrt(dot(v, v)) if MisI else math.sqrt(dot(v, Mv))     # knorm_elliptic(n, v, Mv)
    rNorms = [beta] * nshifts
    if history:
        for i in range(nshifts):
            st.residuals[i].append(rNorms[i])
    ws = SimpleNamespace(x=x, p=None, stats=st, rNorms=rNorms, converged=[False] * nshifts, not_cv=[False] * nshifts,
                         σ=[0.0] * nshifts, δhat=[0.0] * nshifts, ω=[0.0] * nshifts, γ=[0.0] * nshifts)
    if beta == 0:
        st.niter, st.solved = 0, True
        st.status = "x is a zero-residual solution"
        return x, st, ws
    p = [v.copy() for _ in range(nshifts)] if vectors else []           # pᵢ ← v, before v /= β
    ws.p = p
    v *= 1.0 / beta                                                     # kdiv!: kscal! by one(T) / β
    if not MisI:
        Mv *= 1.0 / beta
    Mv_prev = Mv.copy()
    rho = 1.0
    sigma = [beta] * nshifts
    dhat = [0.0] * nshifts
    omega = [0.0] * nshifts
    gamma = [1.0] * nshifts
    eps_tol = atol + rtol * beta
    converged = [r <= eps_tol for r in rNorms]
    not_cv = [not c for c in converged]
    ws.σ, ws.δhat, ws.ω, ws.γ, ws.converged, ws.not_cv = sigma, dhat, omega, gamma, converged, not_cv
    it = 0
    if itmax == 0:
        itmax = 2 * n

    def row():
        return "%5d" % it + "".join("  %8.1e" % r for r in rNorms) + "  %.2fs\n" % (time.perf_counter() - start)
    if verbose > 0 and it % verbose == 0 and out:
        out(row())
    solved = not any(not_cv)
    tired = it >= itmax
    user_exit = overtimed = False
    indefinite = st.indefinite
    while not (solved or tired or user_exit or overtimed):
        Mv_next = mul(v)
        delta = float(dot(v, Mv_next))
        Mv_next = Mv_next - delta * Mv
        if it > 0:
            Mv_next = Mv_next - beta * Mv_prev
            Mv_prev = Mv.copy()
        Mv = Mv_next.copy()
        if MisI:
            v = Mv
            beta = math.sqrt(dot(v, v))
        else:
            v = prec(Mv)
            beta = math.sqrt(dot(v, Mv))
        v *= 1.0 / beta                                                 # v is Mv when M = I
        if not MisI:
            Mv *= 1.0 / beta
            rho = float(dot(v, v))
        for i in range(nshifts):
            dhat[i] = delta + rho * shifts[i]
            gamma[i] = 1.0 / (dhat[i] - omega[i] / gamma[i])
        for i in range(nshifts):
            indefinite[i] = indefinite[i] or gamma[i] <= 0
        for i in range(nshifts):
            not_cv[i] = not (converged[i] or indefinite[i]) if check_curvature else not converged[i]
            if not_cv[i]:
                if vectors:
                    x[i] += gamma[i] * p[i]
                omega[i] = beta * gamma[i]
                sigma[i] *= -omega[i]
                omega[i] *= omega[i]
                if vectors:
                    p[i] = sigma[i] * v + omega[i] * p[i]
                rNorms[i] = abs(sigma[i])
                converged[i] = rNorms[i] <= eps_tol
        if nshifts > 0 and history:
            for i in range(nshifts):
                if not_cv[i]:
                    st.residuals[i].append(rNorms[i])
        for i in range(nshifts):
            not_cv[i] = not (converged[i] or indefinite[i]) if check_curvature else not converged[i]
        it += 1
        if verbose > 0 and it % verbose == 0 and out:
            out(row())
        st.niter = it
        user_exit = bool(callback(ws)) if callback is not None else False
        solved = not any(not_cv)
        tired = it >= itmax
        overtimed = time.perf_counter() - start > timemax
    if verbose > 0 and out:
        out("\n")
    status = "unknown"
    if tired:
        status = "maximum number of iterations exceeded"
    if solved:
        status = "solution good enough given atol and rtol"
    if user_exit:
        status = "user-requested exit"
    if overtimed:
        status = "time limit exceeded"
    st.niter, st.solved, st.status = it, solved, status
    return x, st, ws
