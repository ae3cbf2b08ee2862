"""Test-side NumPy restatement of usymlq! (src/usymlq.jl:124-366, real Float64), line by line, with an injectable `dot` for kdot and
knorm (knorm(x) = sqrt(dot(x, x))).  A checker, not product code: tests/test_usymlq_host.py and tests/test_gpu_usymlq.py compare
the library's three loops with it.  sym_givens and the exactly summed dot are those of tests/bilq_reference.py.

`fault` swaps ONE line for a plausible slip (tests/test_usymlq_host.py shows that the comparison rejects each):
  "alpha_u"      α = ⟨uₖ, q⟩ instead of ⟨vₖ, q⟩
  "one_guard"    one divide guard (βₖ₊₁ ≠ 0) for both vₖ₊₁ and uₖ₊₁
  "zeta_shift"   ζₖ₋₂ is not shifted (it stays 0)
  "dbar_from_v"  d̅ is built from vₖ in place of uₖ
  "cg_no_guard"  the USYMCG residual and test without |δbarₖ| > eps
  "cg_old_dbar"  the USYMCG point is added with d̅ₖ₋₁"""
import math
import time
from types import SimpleNamespace

import numpy as np

from bilq_reference import EPS, _op, fsum_dot, history_deviation, sym_givens  # noqa: F401  (re-exported for the tests)

SOLVED_LQ = "solution xᴸ good enough given atol and rtol"
SOLVED_CG = "solution xᶜ good enough given atol and rtol"
TIRED = "maximum number of iterations exceeded"
ZERO = "x is a zero-residual solution"
FAULTS = ("alpha_u", "one_guard", "zeta_shift", "dbar_from_v", "cg_no_guard", "cg_old_dbar")


def usymlq(A, b, c, x0=None, At=None, transfer_to_usymcg=True, atol=math.sqrt(EPS), rtol=math.sqrt(EPS), itmax=0, timemax=math.inf,
           history=True, callback=None, dot=np.dot, fault=None):
    """A, At: callables v -> op v or objects with `@` (At defaults to A.T); A has m rows and n columns, b has m entries, c has n.
    Returns (x, stats); stats.vectors holds the work vectors by the names of the reference's variables at the end of the loop
    (dbar = d̅ₖ; x_lq = the LQ point before the transfer)."""
    assert fault is None or fault in FAULTS
    start = time.perf_counter()
    mul = _op(A)
    mult = _op(At) if At is not None else (lambda v: A.T @ v)
    norm = lambda v: math.sqrt(float(dot(v, v)))  # noqa: E731
    b = np.asarray(b, dtype=np.float64)
    c = np.asarray(c, dtype=np.float64)
    m, n = b.shape[0], c.shape[0]
    st = SimpleNamespace(niter=0, solved=False, inconsistent=False, status="unknown", residuals=[], vectors={})

    def done(x):
        st.residuals = np.array(st.residuals)
        return x, st

    dx = None if x0 is None else np.asarray(x0, dtype=np.float64)
    r0 = b if dx is None else b - mul(dx)                                    # :150-155
    x = np.zeros(n)
    bNorm = norm(r0)                                                         # :159
    if history:
        st.residuals.append(bNorm)
    if bNorm == 0:                                                           # :161-170
        st.solved, st.status = True, ZERO
        return done(x if dx is None else x + dx)
    it = 0
    if itmax == 0:
        itmax = m + n                                                        # :173
    eps = atol + rtol * bNorm                                                # :175
    beta = norm(r0)                                                          # :179-180
    gamma = norm(c)
    v_prev = np.zeros(m)
    u_prev = np.zeros(n)
    v = r0 / beta
    u = c / gamma
    c_km1 = ck = -1.0                                                        # :185-186
    s_km1 = sk = 0.0
    dbar_vec = np.zeros(n)                                                   # :187
    dbar_vec_old = dbar_vec
    zeta_km1 = zbar = 0.0                                                    # :188-190
    eta_km1 = eta = zeta_km2 = 0.0
    dbar_km1 = dbar = 0.0
    delta_km1 = lam_km1 = eps_km2 = 0.0
    rNorm_cg = math.inf
    q = np.zeros(m)
    p = np.zeros(n)
    solved_lq = bNorm <= eps                                                 # :193-198
    solved_cg = user_exit = overtimed = False
    tired = it >= itmax
    while not (solved_lq or solved_cg or tired or user_exit or overtimed):
        it += 1
        q = mul(u)                                                           # :208-209
        p = mult(v)
        if it >= 2:                                                          # :211-214
            q = q - gamma * v_prev
            p = p - beta * u_prev
        alpha = float(dot(u if fault == "alpha_u" else v, q))                # :216
        q = q - alpha * v                                                    # :218-219
        p = p - alpha * u
        beta_next = norm(q)                                                  # :221-222
        gamma_next = norm(p)
        if it == 1:                                                          # :234-254
            dbar = alpha
        elif it == 2:
            ck, sk, delta_km1 = sym_givens(dbar_km1, gamma)
            lam_km1 = ck * beta + sk * alpha
            dbar = sk * beta - ck * alpha
        else:
            ck, sk, delta_km1 = sym_givens(dbar_km1, gamma)
            eps_km2 = s_km1 * beta
            lam_km1 = -c_km1 * ck * beta + sk * alpha
            dbar = -c_km1 * sk * beta - ck * alpha
        if it == 1:                                                          # :258-260
            eta = beta
        if it == 2:                                                          # :263-266
            zeta_km1 = eta_km1 / delta_km1
            eta = -lam_km1 * zeta_km1
        if it >= 3:                                                          # :270-274
            if fault != "zeta_shift":
                zeta_km2 = zeta_km1
            zeta_km1 = eta_km1 / delta_km1
            eta = -eps_km2 * zeta_km2 - lam_km1 * zeta_km1
        src = v if fault == "dbar_from_v" else u
        dbar_vec_old = dbar_vec
        if it == 1:                                                          # :279-281
            dbar_vec = src.copy()
        else:                                                                # :285-290
            x = x + (zeta_km1 * ck) * dbar_vec
            x = x + (zeta_km1 * sk) * src
            dbar_vec = (-ck) * src + sk * dbar_vec
        v_prev = v                                                           # :294-302
        u_prev = u
        if beta_next != 0:
            v = q / beta_next
        if (beta_next != 0) if fault == "one_guard" else (gamma_next != 0):
            u = p / gamma_next if gamma_next != 0 else np.full(n, math.nan)
        if it == 1:                                                          # :306-312
            rNorm_lq = bNorm
        else:
            mu = beta * (s_km1 * zeta_km2 - c_km1 * ck * zeta_km1) + alpha * sk * zeta_km1
            omega = beta_next * sk * zeta_km1
            rNorm_lq = math.sqrt(mu * mu + omega * omega)
        if history:
            st.residuals.append(rNorm_lq)
        guard = True if fault == "cg_no_guard" else abs(dbar) > EPS
        if transfer_to_usymcg and guard:                                     # :317-321
            with np.errstate(divide="ignore", invalid="ignore"):
                zbar = float(np.float64(eta) / np.float64(dbar))
            rho = beta_next * (sk * zeta_km1 - ck * zbar)
            rNorm_cg = abs(rho)
        s_km1 = sk                                                           # :324-329
        c_km1 = ck
        eta_km1 = eta
        gamma = gamma_next
        beta = beta_next
        dbar_km1 = dbar
        if callback is not None:                                             # :332
            st.niter = it
            user_exit = bool(callback(SimpleNamespace(x=x, stats=st)))
        solved_lq = rNorm_lq <= eps                                          # :333-337
        solved_cg = bool(transfer_to_usymcg and guard and rNorm_cg <= eps)
        tired = it >= itmax
        overtimed = (time.perf_counter() - start) > timemax
    st.vectors = dict(u_prev=u_prev, u=u, p=p, dbar=dbar_vec, v_prev=v_prev, v=v, q=q, x_lq=x)
    if solved_cg:                                                            # :344-346
        x = x + zbar * (dbar_vec_old if fault == "cg_old_dbar" else dbar_vec)
    status = "unknown"                                                       # :349-353
    if tired:
        status = TIRED
    if solved_lq:
        status = SOLVED_LQ
    if solved_cg:
        status = SOLVED_CG
    if user_exit:
        status = "user-requested exit"
    if overtimed:
        status = "time limit exceeded"
    if dx is not None:                                                       # :356
        x = x + dx
    st.niter, st.solved, st.status = it, bool(solved_lq or solved_cg), status
    st.solved_lq, st.solved_cg = bool(solved_lq), bool(solved_cg)
    return done(x)
