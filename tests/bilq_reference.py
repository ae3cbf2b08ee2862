"""Test-side NumPy restatement of bilq! (src/bilq.jl:118-407, real Float64), line by line, with an injectable `dot` for kdot
(knorm(x) = sqrt(dot(x, x))).  A checker, not product code: tests/test_bilq_host.py and tests/test_gpu_bilq.py compare the library's
three loops with it."""
import math
import time
from types import SimpleNamespace

import numpy as np

EPS = np.finfo(np.float64).eps


def fsum_dot(x, y):
    """The exactly rounded dot product of the rounded products: the second opinion the case list is built from."""
    return math.fsum((np.asarray(x, dtype=np.float64) * np.asarray(y, dtype=np.float64)).tolist())


def sym_givens(a, b):
    """sym_givens(a, b) for reals, src/krylov_utils.jl:21-51."""
    sgn = lambda v: 1.0 if v > 0 else (-1.0 if v < 0 else 0.0)  # noqa: E731
    if b == 0:
        return sgn(a) + (1.0 if a == 0 else 0.0), 0.0, abs(a)
    if a == 0:
        return 0.0, sgn(b), abs(b)
    if abs(b) > abs(a):
        t = a / b
        s = sgn(b) / math.sqrt(1.0 + t * t)
        return s * t, s, b / s
    t = b / a
    c = sgn(a) / math.sqrt(1.0 + t * t)
    return c, c * t, a / c


def _op(A):
    return None if A is None else (A if callable(A) else (lambda v: A @ v))


def bilq(A, b, x0=None, c=None, At=None, transfer_to_bicg=True, M=None, N=None, Mt=None, Nt=None, atol=math.sqrt(EPS),
         rtol=math.sqrt(EPS), itmax=0, timemax=math.inf, history=True, callback=None, dot=np.dot):
    """A, At, M, N, Mt, Nt: callables v -> op v or objects with `@` (At defaults to A.T, Mt / Nt to M / N).  Returns (x, stats)."""
    start = time.perf_counter()
    mul = _op(A)
    mult = _op(At) if At is not None else (lambda v: A.T @ v)
    Mop, Nop = _op(M), _op(N)
    Mtop = _op(Mt) if Mt is not None else Mop
    Ntop = _op(Nt) if Nt is not None else Nop
    norm = lambda v: math.sqrt(float(dot(v, v)))  # noqa: E731
    b = np.asarray(b, dtype=np.float64)
    c = b if c is None else np.asarray(c, dtype=np.float64)
    n = b.shape[0]
    st = SimpleNamespace(niter=0, solved=False, inconsistent=False, status="unknown", residuals=[], beta1=0.0)

    def done(x):
        st.residuals = np.array(st.residuals)
        return x, st

    dx = None if x0 is None else np.asarray(x0, dtype=np.float64)
    r0 = b if dx is None else b - mul(dx)
    if Mop is not None:
        r0 = Mop(r0)
    x = np.zeros(n)
    bNorm = norm(r0)
    if history:
        st.residuals.append(bNorm)
    if bNorm == 0:
        st.solved, st.status = True, "x is a zero-residual solution"
        return done(x if dx is None else x + dx)
    it = 0
    if itmax == 0:
        itmax = 2 * n
    cb = float(dot(c, r0))
    if cb == 0:
        st.status = "Breakdown bᴴc = 0"
        return done(x if dx is None else x + dx)
    eps = atol + rtol * bNorm
    beta = math.sqrt(abs(cb))
    st.beta1 = beta                                   # β₁ = sqrt(|cᴴr₀|): equal to ‖r₀‖ only when c = r₀
    gamma = cb / beta
    v_prev = np.zeros(n)
    u_prev = np.zeros(n)
    v = r0 / beta
    u = c / gamma
    c_prev = ck = -1.0
    s_prev = sk = 0.0
    dbar_vec = np.zeros(n)
    zeta_m1 = zbar = 0.0
    eta_prev = eta = zeta_m2 = 0.0
    dbar_prev = dbar = 0.0
    delta = lam = epsilon = 0.0
    norm_v = bNorm / beta
    rNorm_cg = math.inf
    solved_lq = bNorm <= eps
    solved_cg = breakdown = user_exit = overtimed = False
    tired = it >= itmax
    while not (solved_lq or solved_cg or tired or breakdown or user_exit or overtimed):
        it += 1
        Nv = v if Nop is None else Nop(v)
        q = mul(Nv)
        if Mop is not None:
            q = Mop(q)
        Mu = u if Mtop is None else Mtop(u)
        p = mult(Mu)
        if Ntop is not None:
            p = Ntop(p)
        q = q - gamma * v_prev
        p = p - beta * u_prev
        alpha = float(dot(u, q))
        q = q - alpha * v
        p = p - alpha * u
        pq = float(dot(p, q))
        beta_next = math.sqrt(abs(pq))
        gamma_next = pq / beta_next if beta_next != 0 else math.nan
        if it == 1:
            dbar = alpha
        elif it == 2:
            ck, sk, delta = sym_givens(dbar_prev, gamma)
            lam = ck * beta + sk * alpha
            dbar = sk * beta - ck * alpha
        else:
            ck, sk, delta = sym_givens(dbar_prev, gamma)
            epsilon = s_prev * beta
            lam = -c_prev * ck * beta + sk * alpha
            dbar = -c_prev * sk * beta - ck * alpha
        if it == 1:
            eta = beta
        if it == 2:
            zeta_m1 = eta_prev / delta
            eta = -lam * zeta_m1
        if it >= 3:
            zeta_m2 = zeta_m1
            zeta_m1 = eta_prev / delta
            eta = -epsilon * zeta_m2 - lam * zeta_m1
        if it == 1:
            dbar_vec = v.copy()
        else:
            x = x + (zeta_m1 * ck) * dbar_vec
            x = x + (zeta_m1 * sk) * v
            dbar_vec = (-ck) * v + sk * dbar_vec
        v_prev = v
        u_prev = u
        if pq != 0:
            v = q / beta_next
            u = p / gamma_next
        vv_next = float(dot(v_prev, v))
        norm_next = norm(v)
        if it == 1:
            rNorm_lq = bNorm
        else:
            mu = beta * (s_prev * zeta_m2 - c_prev * ck * zeta_m1) + alpha * sk * zeta_m1
            omega = beta_next * sk * zeta_m1
            theta = mu * omega * vv_next
            r2 = mu * mu * norm_v ** 2 + omega * omega * norm_next ** 2 + 2 * theta
            rNorm_lq = math.sqrt(r2) if r2 >= 0 else math.nan
        if history:
            st.residuals.append(rNorm_lq)
        cg_point = transfer_to_bicg and abs(dbar) > EPS
        if cg_point:
            zbar = eta / dbar
            rho = beta_next * (sk * zeta_m1 - ck * zbar)
            rNorm_cg = abs(rho) * norm_next
        s_prev, c_prev, eta_prev = sk, ck, eta
        gamma, beta = gamma_next, beta_next
        dbar_prev = dbar
        norm_v = norm_next
        if callback is not None:
            st.niter = it
            user_exit = bool(callback(SimpleNamespace(x=x, stats=st)))
        solved_lq = rNorm_lq <= eps
        solved_cg = bool(cg_point and rNorm_cg <= eps)
        tired = it >= itmax
        breakdown = (not solved_lq) and (not solved_cg) and pq == 0
        overtimed = (time.perf_counter() - start) > timemax
    if solved_cg:
        x = x + zbar * dbar_vec
    status = "unknown"
    if tired:
        status = "maximum number of iterations exceeded"
    if breakdown:
        status = "Breakdown ⟨uₖ₊₁,vₖ₊₁⟩ = 0"
    if solved_lq:
        status = "solution xᴸ good enough given atol and rtol"
    if solved_cg:
        status = "solution xᶜ good enough given atol and rtol"
    if user_exit:
        status = "user-requested exit"
    if overtimed:
        status = "time limit exceeded"
    if Nop is not None:
        x = Nop(x)
    if dx is not None:
        x = x + dx
    st.niter, st.solved, st.status = it, bool(solved_lq or solved_cg), status
    return done(x)


def history_deviation(h1, h2):
    """Largest relative difference of two residual histories of the same length (inf when the lengths differ)."""
    h1, h2 = np.asarray(h1), np.asarray(h2)
    if h1.shape != h2.shape:
        return math.inf
    return float(np.max(np.abs(h1 - h2) / np.maximum(np.abs(h2), np.finfo(np.float64).tiny)))
