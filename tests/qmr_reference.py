"""Test-side NumPy restatement of qmr! (src/qmr.jl:124-406, real Float64), line by line, with an injectable `dot` for kdot and
kdotr (knorm(x) = sqrt(dot(x, x))).  A checker, not product code: tests/test_qmr_host.py and tests/test_gpu_qmr.py compare the
library's three loops with it.  sym_givens and the exactly summed dot are those of tests/bilq_reference.py."""
import math
import time
from types import SimpleNamespace

import numpy as np

from bilq_reference import EPS, _op, fsum_dot, history_deviation, sym_givens  # noqa: F401  (re-exported for the tests)

SOLVED = "solution good enough given atol and rtol"
TIRED = "maximum number of iterations exceeded"
BREAKDOWN = "Breakdown ⟨uₖ₊₁,vₖ₊₁⟩ = 0"


def qmr(A, b, x0=None, c=None, At=None, M=None, N=None, Mt=None, Nt=None, atol=math.sqrt(EPS), rtol=math.sqrt(EPS), itmax=0,
        timemax=math.inf, history=True, callback=None, dot=np.dot):
    """A, At, M, N, Mt, Nt: callables v -> op v or objects with `@` (At defaults to A.T, Mt / Nt to M / N).  Returns (x, stats);
    stats.vectors holds the work vectors by the names of the reference's variables at the end of the loop."""
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
    st = SimpleNamespace(niter=0, solved=False, inconsistent=False, status="unknown", residuals=[], beta1=0.0, vectors={})

    def done(x):
        st.residuals = np.array(st.residuals)
        return x, st

    dx = None if x0 is None else np.asarray(x0, dtype=np.float64)
    r0 = b if dx is None else b - mul(dx)                                    # :164-167
    if Mop is not None:
        r0 = Mop(r0)                                                         # :168-171
    x = np.zeros(n)
    rNorm = norm(r0)                                                         # :175
    if history:
        st.residuals.append(rNorm)
    if rNorm == 0:                                                           # :178-187
        st.solved, st.status = True, "x is a zero-residual solution"
        return done(x if dx is None else x + dx)
    it = 0
    if itmax == 0:
        itmax = 2 * n
    cb = float(dot(c, r0))                                                   # :193
    if cb == 0:                                                              # :194-203
        st.status = "Breakdown bᴴc = 0"
        return done(x if dx is None else x + dx)
    eps = atol + rtol * rNorm                                                # :205
    beta = math.sqrt(abs(cb))                                                # :209
    st.beta1 = beta                                   # β₁ = sqrt(|cᴴr₀|): equal to ‖r₀‖ only when c = r₀
    gamma = cb / beta
    v_prev = np.zeros(n)
    u_prev = np.zeros(n)
    v = r0 / beta
    u = c / gamma
    c_km2 = c_km1 = ck = 0.0                                                 # :215-216
    s_km2 = s_km1 = sk = 0.0
    w_km2 = np.zeros(n)
    w_km1 = np.zeros(n)
    zbar = beta                                                              # :219
    tau = float(dot(v, v))                                                   # :220
    lbar = eps_km2 = lam = 0.0
    q = np.zeros(n)
    p = np.zeros(n)
    solved = rNorm <= eps
    breakdown = user_exit = overtimed = False
    tired = it >= itmax
    while not (solved or tired or breakdown or user_exit or overtimed):
        it += 1
        Nv = v if Nop is None else Nop(v)                                    # :238-246
        q = mul(Nv)
        if Mop is not None:
            q = Mop(q)
        Mu = u if Mtop is None else Mtop(u)
        p = mult(Mu)
        if Ntop is not None:
            p = Ntop(p)
        q = q - gamma * v_prev                                               # :248-249
        p = p - beta * u_prev
        alpha = float(dot(u, q))                                             # :251
        q = q - alpha * v                                                    # :253-254
        p = p - alpha * u
        pq = float(dot(p, q))                                                # :256
        beta_next = math.sqrt(abs(pq))
        gamma_next = pq / beta_next if beta_next != 0 else math.nan
        if it >= 3:                                                          # :276-281
            eps_km2 = s_km2 * gamma
            lbar = -c_km2 * gamma
        if it >= 2:                                                          # :284-294
            if it == 2:
                lbar = gamma
            lam = c_km1 * lbar + s_km1 * alpha
            dbar = s_km1 * lbar - c_km1 * alpha
            s_km2 = s_km1
            c_km2 = c_km1
        if it == 1:                                                          # :297
            dbar = alpha
        ck, sk, delta = sym_givens(dbar, beta_next)                          # :300
        zeta = ck * zbar                                                     # :307-308
        zbar_next = sk * zbar
        s_km1 = sk                                                           # :311-312
        c_km1 = ck
        if it == 1:                                                          # :316-319
            w_km1 = v / delta
            wk = w_km1
        if it == 2:                                                          # :321-326
            wk = w_km2 + (-lam) * w_km1
            wk = wk + 1.0 * v
            wk = wk * (1.0 / delta)                                          # kdiv! = kscal!(one(T) / δ), src/krylov_utils.jl:325
            w_km2 = wk
        if it >= 3:                                                          # :328-334
            wk = (-eps_km2) * w_km2
            wk = wk + (-lam) * w_km1
            wk = wk + 1.0 * v
            wk = wk * (1.0 / delta)
            w_km2 = wk
        x = x + zeta * wk                                                    # :338
        v_prev = v                                                           # :341-342
        u_prev = u
        if pq != 0:                                                          # :344-347
            v = q / beta_next
            u = p / gamma_next
        tau_next = tau + float(dot(v, v))                                    # :350
        rNorm = abs(zbar_next) * math.sqrt(tau_next)                         # :353
        if history:
            st.residuals.append(rNorm)
        if it >= 2:                                                          # :357-359
            w_km2, w_km1 = w_km1, w_km2
        zbar, beta, gamma, tau = zbar_next, beta_next, gamma_next, tau_next  # :362-365
        resid_decrease_mach = rNorm + 1.0 <= 1.0                             # :369
        if callback is not None:                                             # :372
            st.niter = it
            user_exit = bool(callback(SimpleNamespace(x=x, stats=st)))
        resid_decrease_lim = rNorm <= eps
        solved = resid_decrease_lim or resid_decrease_mach
        tired = it >= itmax
        breakdown = (not solved) and pq == 0
        overtimed = (time.perf_counter() - start) > timemax
    status = "unknown"                                                       # :384-388
    if tired:
        status = TIRED
    if breakdown:
        status = BREAKDOWN
    if solved:
        status = SOLVED
    if user_exit:
        status = "user-requested exit"
    if overtimed:
        status = "time limit exceeded"
    st.vectors = dict(u_prev=u_prev, u=u, q=q, v_prev=v_prev, v=v, p=p, w_prev2=w_km2, w_prev=w_km1)
    if Nop is not None:                                                      # :391-395
        x = Nop(x)
    if dx is not None:
        x = x + dx
    st.niter, st.solved, st.status = it, bool(solved), status
    return done(x)
