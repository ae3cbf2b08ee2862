"""Test-side NumPy restatement of usymqr! (src/usymqr.jl:130-365, real Float64), line by line, with an injectable `dot` for kdot and
knorm (knorm(x) = sqrt(dot(x, x))).  A checker, not product code: tests/test_usymqr_host.py and tests/test_gpu_usymqr.py compare
the library's three loops with it.  sym_givens and the exactly summed dot are those of tests/bilq_reference.py.

`fault` swaps ONE line for a plausible slip (tests/test_usymqr_host.py shows that the comparison rejects each):
  "alpha_u"    α = ⟨uₖ, q⟩ instead of ⟨vₖ, q⟩
  "c_k"        cₖ instead of cₖ₋₁ in ‖Aᴴrₖ₋₁‖
  "one_guard"  one divide guard (βₖ₊₁ ≠ 0) for both vₖ₊₁ and uₖ₊₁
  "kappa_k2"   κ taken at k = 2
  "w_from_v"   the w recurrence with vₖ in place of uₖ"""
import math
import time
from types import SimpleNamespace

import numpy as np

from bilq_reference import EPS, _op, fsum_dot, history_deviation, sym_givens  # noqa: F401  (re-exported for the tests)

SOLVED = "solution good enough given atol and rtol"
TIRED = "maximum number of iterations exceeded"
ZERO = "x is a zero-residual solution"
FAULTS = ("alpha_u", "c_k", "one_guard", "kappa_k2", "w_from_v")


def usymqr(A, b, c, x0=None, At=None, atol=math.sqrt(EPS), rtol=math.sqrt(EPS), itmax=0, timemax=math.inf, history=True,
           callback=None, dot=np.dot, fault=None):
    """A, At: callables v -> op v or objects with `@` (At defaults to A.T); A has m rows and n columns, b has m entries, c has n.
    Returns (x, stats); stats.vectors holds the work vectors by the names of the reference's variables at the end of the loop."""
    assert fault is None or fault in FAULTS
    start = time.perf_counter()
    mul = _op(A)
    mult = _op(At) if At is not None else (lambda v: A.T @ v)
    norm = lambda v: math.sqrt(float(dot(v, v)))  # noqa: E731
    b = np.asarray(b, dtype=np.float64)
    c = np.asarray(c, dtype=np.float64)
    m, n = b.shape[0], c.shape[0]
    st = SimpleNamespace(niter=0, solved=False, inconsistent=False, status="unknown", residuals=[], Aresiduals=[], vectors={})

    def done(x):
        st.residuals = np.array(st.residuals)
        st.Aresiduals = np.array(st.Aresiduals)
        return x, st

    dx = None if x0 is None else np.asarray(x0, dtype=np.float64)
    r0 = b if dx is None else b - mul(dx)                                    # :153-158
    x = np.zeros(n)
    rNorm = norm(r0)                                                         # :162
    if history:
        st.residuals.append(rNorm)
    if rNorm == 0:                                                           # :164-173
        st.solved, st.status = True, ZERO
        return done(x if dx is None else x + dx)
    it = 0
    if itmax == 0:
        itmax = m + n                                                        # :176
    eps = atol + rtol * rNorm                                                # :178
    kappa = 0.0
    beta = norm(r0)                                                          # :183-184
    gamma = norm(c)
    v_prev = np.zeros(m)
    u_prev = np.zeros(n)
    v = r0 / beta
    u = c / gamma
    c_km2 = c_km1 = ck = 1.0                                                 # :189-190
    s_km2 = s_km1 = sk = 0.0
    w_km2 = np.zeros(n)
    w_km1 = np.zeros(n)
    zbar = beta                                                              # :193
    lbar = eps_km2 = lam = 0.0
    q = np.zeros(m)
    p = np.zeros(n)
    solved = rNorm <= eps
    inconsistent = user_exit = overtimed = False
    tired = it >= itmax
    while not (solved or tired or inconsistent or user_exit or overtimed):
        it += 1
        q = mul(u)                                                           # :211-212
        p = mult(v)
        if it >= 2:                                                          # :214-217
            q = q - gamma * v_prev
            p = p - beta * u_prev
        alpha = float(dot(u if fault == "alpha_u" else v, q))                # :219
        q = q - alpha * v                                                    # :221-222
        p = p - alpha * u
        beta_next = norm(q)                                                  # :224-225
        gamma_next = norm(p)
        if it >= 3:                                                          # :244-249
            eps_km2 = s_km2 * gamma
            lbar = -c_km2 * gamma
        if it >= 2:                                                          # :252-258
            if it == 2:
                lbar = gamma
            lam = c_km1 * lbar + s_km1 * alpha
            dbar = s_km1 * lbar - c_km1 * alpha
        if it == 1:                                                          # :261
            dbar = alpha
        ck, sk, delta = sym_givens(dbar, beta_next)                          # :264
        zeta = ck * zbar                                                     # :271-272
        zbar_next = sk * zbar
        src = v if fault == "w_from_v" else u
        if it == 1:                                                          # :276-279
            w_km1 = src / delta
            wk = w_km1
        if it == 2:                                                          # :281-286
            wk = w_km2 + (-lam) * w_km1
            wk = wk + 1.0 * src
            wk = wk * (1.0 / delta)                                          # kdiv! = kscal!(one(T) / δ), src/krylov_utils.jl:325
            w_km2 = wk
        if it >= 3:                                                          # :288-294
            wk = (-eps_km2) * w_km2
            wk = wk + (-lam) * w_km1
            wk = wk + 1.0 * src
            wk = wk * (1.0 / delta)
            w_km2 = wk
        x = x + zeta * wk                                                    # :298
        rNorm = abs(zbar_next)                                               # :301-302
        if history:
            st.residuals.append(rNorm)
        cg = (ck if fault == "c_k" else c_km1) * gamma_next                  # :305-306
        ArNorm = abs(zbar) * math.sqrt(dbar * dbar + cg * cg)
        if history:
            st.Aresiduals.append(ArNorm)
        v_prev = v                                                           # :309-317
        u_prev = u
        if beta_next != 0:
            v = q / beta_next
        if (beta_next != 0) if fault == "one_guard" else (gamma_next != 0):
            u = p / gamma_next if gamma_next != 0 else np.full(n, math.nan)
        if it >= 2:                                                          # :320-328
            w_km2, w_km1 = w_km1, w_km2
            s_km2 = s_km1
            c_km2 = c_km1
        s_km1 = sk                                                           # :329-333
        c_km1 = ck
        zbar, gamma, beta = zbar_next, gamma_next, beta_next
        if it == (2 if fault == "kappa_k2" else 1):                          # :336
            kappa = atol + rtol * ArNorm
        if callback is not None:                                             # :337
            st.niter = it
            user_exit = bool(callback(SimpleNamespace(x=x, stats=st)))
        solved = rNorm <= eps                                                # :338-342
        inconsistent = (not solved) and ArNorm <= kappa
        tired = it >= itmax
        overtimed = (time.perf_counter() - start) > timemax
    status = "unknown"                                                       # :348-351
    if tired:
        status = TIRED
    if solved:
        status = SOLVED
    if user_exit:
        status = "user-requested exit"
    if overtimed:
        status = "time limit exceeded"
    st.vectors = dict(v_prev=v_prev, v=v, q=q, w_prev2=w_km2, w_prev=w_km1, u_prev=u_prev, u=u, p=p)
    if dx is not None:                                                       # :354
        x = x + dx
    st.niter, st.solved, st.inconsistent, st.status = it, bool(solved), bool(inconsistent), status
    return done(x)
