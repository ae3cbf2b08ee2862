"""Test-side NumPy restatement of minres! (src/minres.jl:164-484, linesearch = false), line by line, with np.dot for kdotr
and np.linalg.norm for knorm.  A checker, not product code: tests/test_minres_host.py and tests/test_gpu_minres.py compare
the library's three loops with it."""
import math
import time
from types import SimpleNamespace

import numpy as np

EPS = np.finfo(np.float64).eps


def minres(A, b, x0=None, M=None, lam=0.0, atol=math.sqrt(EPS), rtol=math.sqrt(EPS), etol=math.sqrt(EPS),
           conlim=1 / math.sqrt(EPS), itmax=0, timemax=math.inf, history=True, callback=None, window=5, dot=np.dot):
    """A, M: callables v -> A v (M: v -> M v, symmetric positive definite) or objects with `@`; dot: kdotr.  Returns (x, stats)."""
    start = time.perf_counter()
    mul = A if callable(A) else (lambda v: A @ v)
    prec = None if M is None else (M if callable(M) else (lambda v: M @ v))
    b = np.asarray(b, dtype=np.float64)
    n = b.shape[0]
    st = SimpleNamespace(niter=0, solved=False, inconsistent=False, status="unknown", residuals=[], Aresiduals=[], Acond=[])
    x = np.zeros(n)
    if x0 is not None:
        dx = np.asarray(x0, dtype=np.float64)
        r1 = mul(dx)
        if lam != 0:
            r1 = r1 + lam * dx
        r1 = b - r1
    else:
        dx = None
        r1 = b.copy()
    r2 = r1.copy()
    v = r2 if prec is None else prec(r1)
    beta1 = float(dot(r1, v))
    if beta1 < 0:
        raise ValueError("Preconditioner is not positive definite")
    if beta1 == 0:
        st.niter, st.solved, st.inconsistent = 1, True, False
        st.status = "x is a zero-residual solution"
        if history:
            st.residuals.append(beta1); st.Aresiduals.append(0.0); st.Acond.append(0.0)
        if dx is not None:
            x = x + dx
        return x, _arrays(st)
    beta1 = math.sqrt(beta1)
    beta = beta1
    oldbeta = dbar = epsln = 0.0
    rNorm = beta1
    if history:
        st.residuals.append(beta1)
    phibar = rhs1 = beta1
    rhs2 = gmax = 0.0
    gmin = math.inf
    cs, sn = -1.0, 0.0
    w1 = np.zeros(n)
    w2 = np.zeros(n)
    ANorm2 = 0.0
    Acond = 0.0
    if history:
        st.Acond.append(Acond)
    ArNorm = 0.0
    if history:
        st.Aresiduals.append(ArNorm)
    xENorm2 = 0.0
    err_lbnd = 0.0
    err_vec = np.zeros(window)
    it = 0
    if itmax == 0:
        itmax = 2 * n
    ctol = 1 / conlim if conlim > 0 else 0.0
    eps_tol = atol + rtol * beta1
    solved = False
    tired = it >= itmax
    ill_cond = False
    ill_cond_mach = ill_cond_lim = False
    zero_resid = rNorm <= eps_tol
    fwd_err = user_exit = overtimed = False
    while not (solved or tired or ill_cond or user_exit or overtimed):
        it += 1
        y = mul(v)
        if lam != 0:
            y = y + lam * v
        y = y * (1.0 / beta)                       # kdiv! = kscal!(one(T) / β)
        if it >= 2:
            y = y + (-beta / oldbeta) * r1
        alpha = float(dot(v, y)) / beta
        y = y + (-alpha / beta) * r2
        delta = cs * dbar + sn * alpha
        if it == 1:
            w = v / beta
            w2 = w
        else:
            w = w1
            if it >= 3:
                w = -epsln * w
            w = w + (-delta) * w2
            w = w + (1.0 / beta) * v
        r1 = r2.copy()
        r2 = y.copy()
        v = r2 if prec is None else prec(r2)
        oldbeta = beta
        beta = float(dot(r2, v))
        if beta < 0:
            raise ValueError("Preconditioner is not positive definite")
        beta = math.sqrt(beta)
        ANorm2 = ANorm2 + alpha * alpha + oldbeta * oldbeta + beta * beta
        gbar = sn * dbar - cs * alpha
        epsln = sn * beta
        dbar = -cs * beta
        root = math.sqrt(gbar * gbar + dbar * dbar)
        ArNorm = phibar * root
        if history:
            st.Aresiduals.append(ArNorm)
        gamma = max(math.sqrt(gbar * gbar + beta * beta), EPS)
        w = w * (1.0 / gamma)
        cs = gbar / gamma
        sn = beta / gamma
        phi = cs * phibar
        phibar = sn * phibar
        x = x + phi * w
        xENorm2 = xENorm2 + phi * phi
        if it == 1:
            w2 = w
        else:
            w1, w2 = w2, w
        err_vec[it % window] = phi
        if it >= window:
            err_lbnd = float(np.linalg.norm(err_vec))
        gmax = max(gmax, gamma)
        gmin = min(gmin, gamma)
        zeta = rhs1 / gamma
        rhs1 = rhs2 - delta * zeta
        rhs2 = -epsln * zeta
        ANorm = math.sqrt(ANorm2)
        xNorm = float(np.linalg.norm(x))
        rNorm = phibar
        test1 = rNorm / (ANorm * xNorm)
        test2 = root / ANorm
        if history:
            st.residuals.append(rNorm)
        Acond = gmax / gmin
        if history:
            st.Acond.append(Acond)
        if it == 1 and beta / beta1 <= 10 * EPS:
            st.niter, st.solved, st.inconsistent = 1, True, True
            st.status = "x is a minimum least-squares solution"
            if dx is not None:
                x = x + dx
            return x, _arrays(st)
        ill_cond_mach = 1.0 + 1.0 / Acond <= 1.0
        solved_mach = 1.0 + test2 <= 1.0
        zero_resid_mach = 1.0 + test1 <= 1.0
        resid_decrease_mach = rNorm + 1.0 <= 1.0
        tired = it >= itmax
        ill_cond_lim = 1.0 / Acond <= ctol
        solved_lim = test2 <= eps_tol
        zero_resid_lim = (prec is None) and (test1 <= EPS)
        resid_decrease_lim = rNorm <= eps_tol
        if it >= window:
            fwd_err = err_lbnd <= etol * math.sqrt(xENorm2)
        user_exit = bool(callback(x)) if callback is not None else False
        zero_resid = zero_resid_mach or zero_resid_lim
        resid_decrease = resid_decrease_mach or resid_decrease_lim
        ill_cond = ill_cond_mach or ill_cond_lim
        solved = solved_mach or solved_lim or zero_resid or fwd_err or resid_decrease
        overtimed = time.perf_counter() - start > timemax
    status = "unknown"
    if tired: status = "maximum number of iterations exceeded"
    if ill_cond_mach: status = "condition number seems too large for this machine"
    if ill_cond_lim: status = "condition number exceeds tolerance"
    if solved: status = "found approximate minimum least-squares solution"
    if zero_resid: status = "found approximate zero-residual solution"
    if fwd_err: status = "truncated forward error small enough"
    if user_exit: status = "user-requested exit"
    if overtimed: status = "time limit exceeded"
    if dx is not None:
        x = x + dx
    st.niter, st.solved, st.inconsistent, st.status = it, solved, not zero_resid, status
    return x, _arrays(st)


def _arrays(st):
    st.residuals = np.array(st.residuals)
    st.Aresiduals = np.array(st.Aresiduals)
    st.Acond = np.array(st.Acond)
    return st
